"""The device Viterbi decoders (csrc/viterbi_dev.h) against the oracle's
decode_soft, directly: aero_device_viterbi hands each of them the streams of
tests/viterbi_inputs.py (noisy, hard-valued, tied and erased; every codeword
length production decodes) and every bit of every codeword must equal the
oracle's.  tests/test_viterbi_inputs.py shows on the CPU that these bytes
reach the ACS tie rule, the search's tie rule, the renormalisation, the
start state of the windowed traceback and the restricted tail."""
import numpy as np
import pytest

import aero_testlib as tl  # noqa: F401  (puts the package on sys.path)
import viterbi_inputs as vi


@pytest.fixture(scope='module')
def eng(engine_lib):
    import aero_engine as ae
    e = ae.Engine(max_channels=1)
    yield e
    e.close()


def _differing(nsoft, names, got, ref):
    """[(length, generator, seed, first differing bit)] of the rows that differ."""
    return [(nsoft,) + tuple(names[i]) + (int(np.flatnonzero(got[i] != ref[i])[0]),)
            for i in np.flatnonzero((got != ref).any(axis=1))]


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['wave', 'regs', 'regs2-self'])
def test_decoder_equals_oracle(eng, variant):
    """All lengths x all generators x 8 seeds, one batch per length."""
    bad = []
    for nsoft in vi.LENGTHS:
        names, rows = vi.streams(nsoft)
        got = eng.device_viterbi(variant, rows)
        assert got.shape == (len(names), nsoft // 2)
        bad += _differing(nsoft, names, got, vi.oracle_bits(nsoft))
    assert not bad, '%s: %d codewords differ from the oracle, first %s' % (variant, len(bad), bad[:8])


def _pairings(names):
    """(A, B) row pairs from different generators: every row with the row 11
    further on (generators take at most 8 consecutive rows), and the pairings
    whose halves are furthest apart: an all-ties codeword beside a noisy one
    (metrics near 32640 per renormalisation interval beside small ones), hard
    beside uniform, all0 beside all255."""
    at = {n: i for i, n in enumerate(names)}
    n = len(names)
    pairs = [(i, (i + 11) % n) for i in range(n)]
    for s in vi.SEEDS:
        pairs += [(at['all128', 0], at['noise1.0', s]), (at['hard', s], at['uniform', s])]
    pairs.append((at['all0', 0], at['all255', 0]))
    assert all(names[a][0] != names[b][0] for a, b in pairs)
    return pairs


@pytest.mark.gpu
def test_paired_decoder_halves_are_independent(eng):
    """viterbi_decode_regs2 with two different codewords in the 16-bit halves
    of its registers, each pairing both ways round: each output equals the
    oracle's decode of that codeword alone, and what the same decoder gives
    for the codeword paired with itself (no carry, borrow or compare leaks
    from one half into the other)."""
    bad = []
    for nsoft in vi.LENGTHS:
        names, rows = vi.streams(nsoft)
        order = np.array([k for a, b in _pairings(names) for k in (a, b, b, a)])
        got = eng.device_viterbi('regs2-pair', rows[order])
        alone = eng.device_viterbi('regs2-self', rows)
        onames = [names[k] + ('beside',) + names[p] for k, p in zip(order, order.reshape(-1, 2)[:, ::-1].ravel())]
        for ref in (vi.oracle_bits(nsoft)[order], alone[order]):
            bad += [(nsoft, onames[i]) for i in np.flatnonzero((got != ref).any(axis=1))]
    assert not bad, '%d paired codewords differ, first %s' % (len(bad), bad[:8])


@pytest.mark.gpu
def test_odd_batch_decodes_its_last_codeword(eng):
    """An odd regs2-pair batch: the last codeword has no partner."""
    names, rows = vi.streams(662)
    got = eng.device_viterbi('regs2-pair', rows[:5])
    assert np.array_equal(got, vi.oracle_bits(662)[:5])


# ------------------------------------------------------- production sources
def _interleave(d, blk):
    """The raw block whose deinterleave (position 64 j + l from row (27 l) mod 64, column j) is d."""
    q = np.arange(blk)
    raw = np.zeros(blk, dtype=np.uint8)
    raw[(((q & 63) * 27) & 63) * (blk // 64) + (q >> 6)] = d
    return raw


def _host_stream(rec, blk, first, cchan):
    """What the decoder is to see of a record: the overlap (unless first), the
    block deinterleaved (C: the frame with erasures at 4 k + 3), 24 erasures."""
    raw = rec[:blk]
    if cchan:
        d = raw.copy()
        d[3::4] = 128
    else:
        q = np.arange(blk)
        d = raw[(((q & 63) * 27) % 64) * (blk // 64) + (q >> 6)]
    return np.concatenate([rec[blk:blk + 62][:0 if first else 62], d, np.full(24, 128, dtype=np.uint8)])


def _records(blk, first, cchan, rng):
    """Random and adversarial raw blocks with their overlap bytes: structureless
    blocks, and noisy codewords laid out so that the source's own reordering
    (and, for C, its erasures) gives back a decodable stream."""
    ov = 0 if first else 62
    nsoft = ov + blk + 24
    recs = []

    def add(raw, overlap):
        rec = np.zeros(blk + 64, dtype=np.uint8)
        rec[:blk], rec[blk:blk + 62], rec[blk + 62] = raw, overlap, first
        recs.append(rec)

    def overlap():  # random, with 0, 128 and 255 among them (for a first block: never read)
        o = rng.integers(0, 256, 62)
        o[rng.integers(0, 62, 15)] = rng.choice([0, 128, 255], 15)
        return o

    for _ in range(6):
        add(rng.integers(0, 256, blk), overlap())
    for _ in range(4):
        add(rng.integers(0, 2, blk) * 255, overlap())
        add(rng.choice([0, 128, 255], blk), overlap())
    for _ in range(2):
        add(rng.choice([127, 128, 129], blk), overlap())
    for v in (0, 128, 255):
        add(np.full(blk, v), np.full(62, v))
        add(np.full(blk, v), overlap())
    for sigma in (0.5, 1.0, 1.0, 1.3, 1.3):
        x = 2.0 * vi.encoded_bits(rng, nsoft) - 1.0 + rng.normal(0, sigma, nsoft)
        s = np.clip(np.round(x * 0.75 * 127 + 128), 0, 255).astype(np.uint8)
        d = s[ov:ov + blk]
        add(d if cchan else _interleave(d, blk), s[:62])  # C: the values at 4 k + 3 stay, to be erased by the source
    assert len(recs) % 2 == 1  # the last block decodes without a partner
    return nsoft, np.stack(recs)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['block4992', 'block384', 'block576', 'csoft'])
def test_production_sources(eng, variant):
    """viterbi_decode_regs2 reading through BlockSoft<BLK> / CSoft, built as the
    continuous channels' kernels build them, for a stream's first block and a
    continuing one: decoded bits against the oracle's decode of the stream the
    host assembles, and the 62 overlap values handed to the next block."""
    import aero_engine as ae
    blk, cchan = ae.VIT_BLOCK[variant], variant == 'csoft'
    rng = np.random.default_rng([0xAE71, blk])
    for first in (1, 0):
        nsoft, recs = _records(blk, first, cchan, rng)
        assert nsoft in (vi.C_LENGTHS if cchan else vi.BLOCK_LENGTHS[blk])
        bits, ovl = eng.device_viterbi(variant, recs, nsoft)
        streams = np.stack([_host_stream(r, blk, first, cchan) for r in recs])
        assert streams.shape[1] == nsoft
        ref = np.stack([vi.oracle_decode(s) for s in streams])
        bad = np.flatnonzero((bits != ref).any(axis=1))
        assert not len(bad), '%s first=%d: records %s differ from the oracle' % (variant, first, bad.tolist())
        assert np.array_equal(ovl, streams[:, nsoft - 24 - 62:nsoft - 24]), '%s first=%d: overlap' % (variant, first)


@pytest.mark.gpu
def test_probe_refuses_what_it_cannot_run(eng):
    import aero_engine as ae
    ok = np.full((2, 128), 128, dtype=np.uint8)
    for variant, rows, nsoft in (('regs', ok[:, :127], None), ('wave', ok[:, :22], None),
                                 ('regs2-self', np.zeros((1, 6082), dtype=np.uint8), None),
                                 ('block384', np.zeros((1, 448), dtype=np.uint8), 409),
                                 ('block384', np.zeros((1, 448), dtype=np.uint8), 408)):  # first = 0 says 470
        with pytest.raises(ae.AeroError) as ei:
            eng.device_viterbi(variant, rows, nsoft)
        assert ei.value.rc == ae.AERO_E_INVALID
