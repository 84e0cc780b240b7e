"""Seeded soft-decision streams for the K=7 Viterbi decoders: the input set
tests/test_viterbi_inputs.py proves strong on the CPU (every mutation of the
oracle's decoder changes an output bit) and tests/test_gpu_viterbi.py feeds
to the device decoders.  Same bytes in both: a stream depends on its
generator, its seed and its length only.

The synthetic streams' soft bits are nearly saturated, so the decoder's tie
rules, its renormalisation and its restricted tail never decide a bit there;
these inputs are noisy, hard-valued or erased so that they do."""
import functools

import numpy as np

import aero_testlib as tl

# every codeword length production decodes, and nothing larger
RT_LENGTHS = [128] + [320 + 192 * k for k in range(31)]  # R/T tests (burst.hip frame kernel: 128, then 320 + 192 k)
BLOCK_LENGTHS = {384: (408, 470), 576: (600, 662), 4992: (5016, 5078)}  # BLK: first block, continuing block
C_LENGTHS = (5484, 5546)
LENGTHS = sorted(set(RT_LENGTHS) | {n for v in BLOCK_LENGTHS.values() for n in v} | set(C_LENGTHS))

SEEDS = tuple(range(8))
HCAP, MINTB, RENORM, TBGROUP = 140, 35, 128, 105  # history columns, traceback depth, renormalisation, columns per traceback

NOISE_SIGMAS = (0.5, 0.8, 1.0, 1.3)
SEEDED = ['noise%.1f' % s for s in NOISE_SIGMAS] + ['uniform', 'hard', 'hard12pct', 'tern', 'near128', 'bursterr']
FIXED = ['all128', 'all0', 'all255', 'alt']


def columns(nsoft):
    """History columns of a codeword (one per trellis step after the warmup)."""
    return nsoft // 2 - 6


def windowed_tracebacks(nsoft):
    """Column counts at which a traceback leaves the 35-column depth: the
    history is full at 140 columns and gives 105 away each time."""
    return list(range(HCAP, columns(nsoft) + 1, TBGROUP))


def encoded_bits(rng, nsoft, message=False):
    """nsoft code bits of a random message of nsoft/2 - 6 bits and its zero
    tail; with `message` also the message bits."""
    sets = nsoft // 2
    bits = rng.integers(0, 2, 8 * ((sets + 7) // 8), dtype=np.uint8)
    bits[sets - 6:] = 0  # the encoder's own tail follows the last byte; these zeros are the codeword's
    msg = np.packbits(bits)
    enc = np.zeros(2 * (len(msg) + 1) + 8, dtype=np.uint8)
    n = tl.Oracle.lib().oracle_conv_encode(msg.ctypes.data, len(msg), enc.ctypes.data)
    assert n >= nsoft
    code = np.unpackbits(enc)[:nsoft]
    return (code, bits[:sets - 6]) if message else code


def burst_columns(nsoft):
    """Columns a `bursterr` run is centred on: the first step, a 64-column
    register edge and the 64-step refill of the buffered soft pairs (64), the
    renormalisation and the second register edge (128), the history's wrap and
    the first traceback (140), the second refill (192), the second traceback
    (245 = 140 + 105) and the last 6 steps."""
    cols = columns(nsoft)
    return sorted({c for c in (0, 64, 128, 140, 192, 245) if c < cols} | {cols - 3})


def _stream(name, seed, nsoft):
    rng = np.random.default_rng([0xAE70, (SEEDED + FIXED).index(name), seed, nsoft])
    if name.startswith('noise'):
        x = 2.0 * encoded_bits(rng, nsoft) - 1.0 + rng.normal(0, float(name[5:]), nsoft)
        return np.clip(np.round(x * 0.75 * 127 + 128), 0, 255)
    if name == 'uniform':
        return rng.integers(0, 256, nsoft)
    if name == 'hard':
        return rng.integers(0, 2, nsoft) * 255
    if name == 'hard12pct':
        return (encoded_bits(rng, nsoft) ^ (rng.integers(0, 8, nsoft) == 0)) * 255
    if name == 'tern':
        return rng.choice([0, 128, 255], nsoft)
    if name == 'near128':  # |128 - 0| != |128 - 255|
        return rng.choice([127, 128, 129], nsoft)
    if name == 'bursterr':
        # 100 inverted values (longer than the traceback depth) around every
        # fourth event boundary; four seeds cover all of them
        s = encoded_bits(rng, nsoft) * 255
        for c in burst_columns(nsoft)[seed % 4::4]:
            mid = 2 * (c + 6)
            lo, hi = max(0, mid - 50), min(nsoft, mid + 50)
            s[lo:hi] = 255 - s[lo:hi]
        return s
    if name == 'all128':  # every branch costs 255: the tie rules alone decide, and the metrics grow fastest
        return np.full(nsoft, 128)
    if name == 'all0':
        return np.zeros(nsoft)
    if name == 'all255':
        return np.full(nsoft, 255)
    if name == 'alt':
        return np.tile([0, 255], nsoft // 2)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def streams(nsoft):
    """(names, uint8 array [n, nsoft]): every seeded generator at every seed,
    then the fixed streams.  names[i] = (generator, seed)."""
    names = [(g, s) for g in SEEDED for s in SEEDS] + [(g, 0) for g in FIXED]
    rows = np.stack([np.asarray(_stream(g, s, nsoft)).astype(np.uint8) for g, s in names])
    rows.setflags(write=False)
    return names, rows


def oracle_decode(soft, mut=0):
    """The oracle's decode of one stream as nsoft/2 bits (the nsoft/2 - 6
    decoded bits, then zeros); mut: oracle_viterbi_decode_soft_mut's switch."""
    L = tl.Oracle.lib()
    soft = np.ascontiguousarray(soft, dtype=np.uint8)
    out = np.zeros(len(soft) // 16 + 8, dtype=np.uint8)
    if mut:
        L.oracle_viterbi_decode_soft_mut(soft.ctypes.data, len(soft), out.ctypes.data, mut)
    else:
        L.oracle_viterbi_decode_soft(soft.ctypes.data, len(soft), out.ctypes.data)
    return np.unpackbits(out)[:len(soft) // 2]


@functools.lru_cache(maxsize=None)
def oracle_bits(nsoft):
    """The oracle's decode of streams(nsoft), [n, nsoft/2]; computed once, read-only."""
    ref = np.stack([oracle_decode(r) for r in streams(nsoft)[1]])
    ref.setflags(write=False)
    return ref
