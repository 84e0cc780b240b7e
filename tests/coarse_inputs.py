"""Short int16 streams for the coarse estimator's smoothed spectrum y
(tests/test_coarse_inputs.py proves on the CPU, with the oracle alone, which
paths they reach; tests/test_gpu_coarse_y.py compares the engine's y with the
oracle's after every run()).  Each stream is a whole number of hops plus a
remainder.  A hunter step needs 15 signal-less hops (Hunter::maxTries), so
the silent classes run silent_hops(mode) hops (17 for OQPSK and C; see
STEP_HOP); 6 hops are enough for the others, and the classes that need the
hunter's step first take silent_hops + 6."""
import functools

import numpy as np

import aero_testlib as tl

SEED = 0xC0A5
TAIL = 37  # samples behind the last whole hop

# name: AeroL bit rate, sample rate, hop, nfft, lockingbw (Decoder's settings)
MODES = {
    'oqpsk10500@48000': (10500, 48000, 4096, 16384, 10500.0),
    'c8400@48000': (8400, 48000, 4096, 16384, 10500.0),
    'msk600@12000': (600, 12000, 2048, 8192, 900.0),
    'msk600@24000': (600, 24000, 2048, 8192, 900.0),
    'msk600@48000': (600, 48000, 2048, 8192, 900.0),
    'msk1200@12000': (1200, 12000, 2048, 8192, 900.0),
    'msk1200@24000': (1200, 24000, 2048, 8192, 900.0),
    'msk1200@48000': (1200, 48000, 2048, 8192, 900.0),
    'msk600@22050': (600, 22050, 2048, 8192, 900.0),
}
HOPS = 6
# The hunter steps after 15 signal-less hops (Hunter::maxTries).  OQPSK and C
# count from the first hop; the MSK demodulator starts with mse = 10 behind a
# 600-sample average of a detector that needs some symbols, which the oracle
# reports as "signal" for 2, 5 or 11 hops of 2048 samples at 12, 24 (22.05)
# and 48 kHz.  STEP_HOP: the hop in which a silent channel takes its first
# step (tests/test_coarse_inputs.py checks it); the silent classes run two
# hops longer.
STEP_HOP = {'oqpsk10500@48000': 15, 'c8400@48000': 15, 'msk600@12000': 17, 'msk1200@12000': 17,
            'msk600@24000': 20, 'msk1200@24000': 20, 'msk600@22050': 20, 'msk600@48000': 26, 'msk1200@48000': 26}


def silent_hops(mode):
    return STEP_HOP[mode] + 2


# silence and full scale are neighbours: what one leaves in LDS is as unlike
# the other's values as it can be
ORDER = ('silence', 'square', 'one_sample', 'const_min', 'lsb_noise', 'tone', 'noise', 'edge_lo', 'edge_hi',
         'silence_carrier', 'reset_silence')
# the bins of y the engine keeps (what the fold reads), by nfft
KEPT = {16384: (2815, 13568), 8192: (3276, 4915)}


def fold_range(mode):
    """[ILO, IHI) of the fold search and Hz per bin (coarsefreqestimate.cpp:113-116)."""
    _, fs, _, nfft, bw = MODES[mode]
    hz = fs / nfft
    return int(round(-bw / hz + nfft / 2)), int(round(bw / hz + nfft / 2)), hz


def edge_est(mode, edge):
    """freq_offset_est of a fold peak in the first ('lo') / last ('hi') bin of the search range."""
    ilo, ihi, hz = fold_range(mode)
    _, _, _, nfft, _ = MODES[mode]
    return -((ilo if edge == 'lo' else ihi - 1) - nfft / 2) * hz * 0.5


def oracle(mode):
    bitrate, fs = MODES[mode][:2]
    return tl.Oracle(bitrate=bitrate)


def push(o, mode, pcm):
    """One message into an oracle channel of this mode (MSK: at the mode's rate)."""
    bitrate, fs = MODES[mode][:2]
    o.push(pcm, fs if bitrate in (600, 1200) else None)


def _carrier(mode, f, n, seed, lead=None):
    bitrate, fs = MODES[mode][:2]
    sec = n / fs + 0.01
    if bitrate == 10500:
        x = tl.synth(seconds=sec, seed=seed, carrier=f, ebn0=12.0, lead_in=1000 if lead is None else lead)
    elif bitrate == 8400:
        x = tl.synth_c(seconds=sec, seed=seed, carrier=f, ebn0=12.0, lead_in=1000 if lead is None else lead)
    else:
        x = tl.synth_msk(seconds=sec, bitrate=bitrate, seed=seed, carrier=f, ebn0=12.0, lead_in=500 if lead is None else lead, fs=fs)
    assert len(x) >= n
    return x[:n]


def push_hops(o, mode, pcm):
    """The stream one hop per message (the C channel's output depends on the
    message boundaries: its prefilter runs per message)."""
    hop = MODES[mode][2]
    for k in range(0, len(pcm), hop):
        push(o, mode, pcm[k:k + hop])


def _reaches(mode, pcm, want):
    o = oracle(mode)
    push_hops(o, mode, pcm)
    return bool((o.hops()[:, 1] == want).any())


@functools.lru_cache(maxsize=None)
def edge_stream(mode, edge):
    """A stream whose fold peak the oracle finds in the first ('lo') / last
    ('hi') bin of the search range in one of its hops.

    OQPSK: a tl.synth carrier half the locking bandwidth from the
    estimator's first centre, 0 Hz (a real carrier at f shows at +f and -f
    there), searched outwards in eighths of a bin; 6 hops.

    C and MSK: around 0 Hz the spectrum of a real signal is symmetric, so the
    last bin can only tie with a lower one, and a synth carrier near the edge
    loses to its own image fb / 2 away (the oracle answers 2100 Hz and 150 Hz
    there).  So: silence until the hunter has stepped (to 5250 or 450 Hz),
    then two tones whose squares put lines fb / 2 below and above the edge
    bin, searched over neighbouring tone bins; silent_hops + 6 hops."""
    bitrate, fs, hop, nfft, bw = MODES[mode]
    hz = fs / nfft
    want = edge_est(mode, edge)
    n = HOPS * hop + TAIL
    if bitrate == 10500:
        for k in range(0, 41):
            for f in ((bw / 2 + k * hz / 8, bw / 2 - k * hz / 8) if k else (bw / 2,)):
                pcm = _carrier(mode, f, n, SEED + 7, lead=0)  # modulated from the first sample
                if _reaches(mode, pcm, want):
                    return pcm
    else:
        # Hunter: minFreq + (bandwidth >> 1) (MSK: CenterFreqChangedSlot's lower clamp as well); fb stays 600 for MSK
        centre, fb = (5250.0, 8400.0) if bitrate == 8400 else (450.0, 600.0)
        ilo, ihi, _ = fold_range(mode)
        epb = int(round(fb / (2.0 * hz)))
        i = (ilo if edge == 'lo' else ihi - 1) - nfft // 2  # the edge bin from the centre of the shifted spectrum
        t = np.arange(n)
        for da in (0, 1, -1, 2, -2):
            for db in (0, 1, -1, 2, -2):
                a, b = (i - epb) // 2 + da, (i + epb) // 2 + db  # baseband tone bins: their squares' lines at 2a, 2b
                x = sum(np.cos(2 * np.pi * (centre - k * hz) / fs * t) for k in (a, b))  # the mix mirrors the spectrum
                pcm = np.concatenate([np.zeros(silent_hops(mode) * hop, dtype=np.int16),
                                      np.round(6000 * x).astype(np.int16)])
                if _reaches(mode, pcm, want):
                    return pcm
    raise AssertionError('%s: no stream puts the fold peak on the %s edge' % (mode, edge))


RESET_TAIL_HOPS = 5  # bigchange() holds the estimate at 0 for 4 hops (emptyingcountdown); the fifth shows it


@functools.lru_cache(maxsize=None)
def reset_stream(mode):
    """OQPSK and C: silence until the hunter has stepped, a carrier 40 Hz off
    the new centre until the AFC retunes (five hops with a signal more than
    3 Hz off: mixer_center moves, bigchange() sets y = 20 and clears the
    snapshot), then silence: y is 20, then 18, ... in every bin, every fold
    sum ties and the first bin of the search range wins.  (stream, the hop
    that ends with the reset).  The MSK demodulator's AFC branch needs dcd,
    which nothing sets (mskdemodulator.cpp:430-469): no reset there, no
    such class."""
    bitrate, fs, hop, nfft, bw = MODES[mode]
    if bitrate not in (10500, 8400):
        return None, None
    lead = np.zeros(silent_hops(mode) * hop, dtype=np.int16)
    car = _carrier(mode, 5250.0 + 40.0, 16 * hop, SEED + 9)
    o = oracle(mode)
    push_hops(o, mode, lead)
    for k in range(16):
        push(o, mode, car[k * hop:(k + 1) * hop])
        y = o.coarse_y()
        if y.min() == 20.0 and y.max() == 20.0:
            r = silent_hops(mode) + k + 1
            assert len(o.hops()) == r
            return np.concatenate([lead, car[:(k + 1) * hop], np.zeros(RESET_TAIL_HOPS * hop + TAIL, dtype=np.int16)]), r
    raise AssertionError('%s: the AFC never retuned' % mode)


@functools.lru_cache(maxsize=None)
def streams(mode):
    """[(class, int16 stream)] in ORDER (reset_silence: OQPSK and C only)."""
    _, fs, hop, nfft, bw = MODES[mode]
    rng = np.random.default_rng([SEED, fs, hop])
    ns, n = silent_hops(mode) * hop + TAIL, HOPS * hop + TAIL
    out = {}
    out['silence'] = np.zeros(ns, dtype=np.int16)
    sq = np.where((np.arange(n) // 3) % 2 == 0, 32767, -32768).astype(np.int16)
    out['square'] = sq
    one = np.zeros(ns, dtype=np.int16)
    one[hop + hop // 2] = 29
    out['one_sample'] = one
    out['const_min'] = np.full(n, -32768, dtype=np.int16)
    out['lsb_noise'] = rng.integers(-1, 2, ns).astype(np.int16)
    kbin = int(bw / 4 / (fs / nfft))  # an exact bin centre inside the first search window
    out['tone'] = np.round(8192 * np.cos(2 * np.pi * ((kbin * np.arange(n)) % nfft) / nfft)).astype(np.int16)
    out['noise'] = np.clip(np.round(rng.normal(0, 0.25 * 32768 / 3, n)), -32768, 32767).astype(np.int16)
    out['edge_lo'] = edge_stream(mode, 'lo')
    out['edge_hi'] = edge_stream(mode, 'hi')
    # the hunter's first step goes to half its bandwidth; the carrier waits there
    fstep = (10500 >> 1) if bw > 900 else (900 >> 1)
    out['silence_carrier'] = np.concatenate([np.zeros(silent_hops(mode) * hop, dtype=np.int16),
                                             _carrier(mode, fstep + 40.0 * fs / 48000, n, SEED + 9)])
    out['reset_silence'] = reset_stream(mode)[0]
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return [(name, out[name]) for name in ORDER if out[name] is not None]
