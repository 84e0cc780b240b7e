"""Adversarial int16 streams for the continuous demodulators (demod_oqpsk.hip,
demod_msk.hip, cchan.hip): tests/test_cont_inputs.py proves on the CPU, with
the oracle and its range probe (tools/oracle_ranges.cpp), which of the
kernels' fast-path limits the classes reach; tests/test_gpu_cont_inputs.py
compares everything the engine delivers with the oracle's after every run().

A stream is a whole number of hops and a 37-sample tail.  The silent classes
(SILENT) take coarse_inputs.silent_hops(mode) hops, so the hunter steps;
`two_samples` takes as long as its second sample needs; the locking classes
(LOCKING) take the shortest length, in whole hops, at which the oracle, fed
one hop per message, has a DataCarrierDetect rise and a frame with a good CRC
(C: and a Call_progress SU); the cut_* classes run until the ticked oracle's
DataCarrierDetect has fallen again (CUT_FALL_SECONDS at most); the rest take
6 hops.  A search that finds nothing raises AssertionError.

msk600@48000 drops the good-frame requirement and keeps the rise (NO_FRAME):
its first good frame lies more than 400000 samples into the stream (none
within 200 hops), over 3 s of a lane's time for every locking class in every
engine of the GPU test.

The AGC ring (AGC_LEN) is Fs samples for MSK and 4 Fs = 192000 for OQPSK and
C (AGC(4, 48000)).  It starts as zeros, and a sum of zeros is exactly zero
whatever its length, so `late`, whose carrier finds the gain on its 1e-6
floor, needs no lead longer than the ring: LATE_LEAD is Fs samples and a hop
(past the first DCD timer tick).  `two_samples` is the class that turns the
ring over: its second sample comes after the first has left the ring, when
the ring's sum is the rounding residue of what was added and taken away.

Carriers: 8000 Hz for OQPSK and C, 600 Hz for MSK 600 and 1800 Hz for MSK 1200
(600 baud for both bit rates, what a continuous MSK channel demodulates), at
12 dB Eb/N0, from the synthesisers coarse_inputs and burst_inputs use.  At
24 kHz the oracle's lock is fickle: between 300 and 1350 Hz one of the six
locking classes or another misses its first chance and finds no good frame
within 200 hops; from 1650 Hz on all six lock, with a rise in hop 95 (`late`:
61) and a good frame by hop 142."""
import concurrent.futures as cf
import ctypes
import functools
import itertools

import numpy as np

import aero_testlib as tl
import cont_dcd_lib as cd
import coarse_inputs as ci

SEED = 0xC0A7
TAIL = 37
HOPS = 6

MODES = ('oqpsk10500@48000', 'c8400@48000', 'msk600@12000', 'msk1200@24000', 'msk600@48000', 'msk600@22050')
CARRIER = {'oqpsk10500@48000': 8000.0, 'c8400@48000': 8000.0, 'msk600@12000': 600.0, 'msk1200@24000': 1800.0,
           'msk600@48000': 600.0, 'msk600@22050': 600.0}
SYNTH_SEED = {10500: 5, 8400: 5, 600: 21, 1200: 21}  # by bit rate (21: burst_inputs' MSK stream)
NO_FRAME = ('msk600@48000',)  # locking classes searched for the DCD rise alone
LOCK_HOPS_MAX = 240  # the longest stream a locking class is searched in
CUT_FALL_SECONDS = 6  # how long behind the cut the ticked oracle's fall is searched
FAR_STEP = 62.5  # Hz at 48 kHz (scaled with Fs): the tone grid of the sincos search.  |marg.Val| is sharp in
# frequency (OQPSK: 0.709 at 14250 Hz, 0.080 at 14437.5 Hz), so a coarser grid finds what the grid allows
FAR_BATCH = 32  # candidates probed at a time

# unlike neighbours side by side: silence beside full scale, -32768 beside a
# decoding lane, the cut carriers beside noise
ORDER = ('silence', 'square', 'synth', 'const_min', 'one_sample', 'lsb_noise', 'clip', 'two_samples', 'noise',
         'tone', 'tiny', 'tone_far', 'negated', 'cut_silence', 'lead0', 'cut_fullscale', 'late', 'cut_noise',
         'gated', 'overlap')
SILENT = ('silence', 'one_sample', 'lsb_noise')
LOCKING = ('synth', 'clip', 'tiny', 'negated', 'lead0', 'late')
CUTS = ('cut_silence', 'cut_fullscale', 'cut_noise')

SCHEDULES = ('hop', 'ragged', 'queued')
C_QUEUED = (2049, 32768, 1, 4095, 12000)  # C refuses a message above 32768


def dims(mode):
    """(AeroL bit rate, sample rate, hop)"""
    return ci.MODES[mode][:3]


def is_msk(mode):
    return dims(mode)[0] in (600, 1200)


def agc_len(mode):
    """AGC ring: agc.init(1, Fs) for MSK, AGC(4, 48000) for OQPSK and C"""
    return dims(mode)[1] if is_msk(mode) else 4 * 48000


def late_lead(mode):
    _, fs, hop = dims(mode)
    return fs + hop


def runs(mode, n, schedule):
    """The [start, stop) of every message of an n-sample stream, grouped by
    the run() they are queued before.  hop: one hop per run; ragged: hop - 1,
    hop + 1, 3 hop + 7, 1, 2 hop - 8 cycled (C: aero_testlib.RAGGED, around the
    prefilter's 2048-sample blocks), one per run; queued: five messages per
    run, for OQPSK and MSK with one of 40000 samples, more than half the PCM
    ring, and 77000 (OQPSK) or 67000 (MSK) samples in all, more than the ring
    holds, so that the overrun guard runs the group between two of them."""
    _, _, hop = dims(mode)
    c = dims(mode)[0] == 8400
    if schedule == 'hop':
        sizes, per = (hop,), 1
    elif schedule == 'ragged':
        sizes, per = (tl.RAGGED if c else (hop - 1, hop + 1, 3 * hop + 7, 1, 2 * hop - 8)), 1
    else:
        sizes, per = (C_QUEUED if c else (3 * hop + 7, 40000, 2 * hop + 1, 5000, 12000)), 5
    out, p, k = [], 0, 0
    while p < n:
        grp = []
        for _ in range(per):
            if p < n:
                grp.append((p, min(n, p + sizes[k % len(sizes)])))
                p = grp[-1][1]
                k += 1
        out.append(grp)
    return out


class MskOracle(cd.ContTickOracle):
    """cont_dcd_lib.ContTickOracle with the pt trace"""

    def __init__(self, bitrate, fs, tick):
        tl.Oracle.__init__(self, bitrate=bitrate, trace_pt=True)
        self.tick = tick
        self.clock = cd.TickClock(fs)
        self.fs = fs

    def push(self, pcm, fs=None):
        cd.ContTickOracle.push(self, pcm, self.fs)


def oracle(mode, tick=False):
    """The reference channel of a mode: tl.Oracle with its sample-clock DCD
    timer for OQPSK and C, the hooked oracle cut at the model's tick samples
    for MSK; all with the pt trace."""
    bitrate, fs, _ = dims(mode)
    if is_msk(mode):
        return MskOracle(bitrate, fs, tick)
    return tl.Oracle(bitrate=bitrate, trace_pt=True, dcd_tick=tick)


def outputs(o):
    """everything a continuous channel delivers, in the shape of the engine's accessors"""
    edges, centres = o.events()
    out = dict(pt=o.pt(), hops=o.hops(), soft=o.softbits(), blocks=o.blocks(), frames=o.frames(),
               items=o.item_lines('A'), edges=edges, centres=centres)
    if o.bitrate == 8400:
        out.update(c_units=o.c_units(), voice=o.voice())
    return out


def good_frames(frames):
    return sum(1 for _, mask in tl.frame_records(frames) if mask)


def facts(mode, pcm, schedule='hop', tick=False):
    """What a stream reaches in the oracle, as plain numbers."""
    o = oracle(mode, tick)
    for grp in runs(mode, len(pcm), schedule):
        for a, b in grp:
            o.push(pcm[a:b])
    out = outputs(o)
    return dict(edges=out['edges'], steps=len(out['centres']), soft=len(out['soft']), pt=len(out['pt']),
                frames=good_frames(out['frames']), units=len(out.get('c_units', ())), hops=len(out['hops']),
                finite=bool(np.isfinite(out['pt']).all() and np.isfinite(out['hops']).all()))


# ------------------------------------------------------------------ the range probe
SITES = ('hypot', 'atan2', 'tanh', 'tanh_st', 'sincos', 'mse_hypot', 'div_agc', 'div_tw', 'div_nudge', 'div_m2ptr',
         'div_mssum')  # oracle/aero_oracle.cpp OBS_*
SINCOS_BOUND = 0.855469  # aero_sincos_bf: hi word below 0x3feb6000
_probe = []


def _probe_lib():
    if not _probe:
        import build  # aero-cli_amd/build.py (aero_testlib puts it on the path)
        L = ctypes.CDLL(build.build_oracleranges())
        L.oracle_ranges.restype = ctypes.c_int
        L.oracle_ranges.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                    ctypes.c_void_p]
        _probe.append(L)
    return _probe[0]


def ranges(mode, pcm):
    """{site: (calls, calls outside the kernels' branch-free range or division
    contract, calls with a nonzero subnormal argument, largest |argument|)} of
    the stream fed one hop per message"""
    bitrate, fs, hop = dims(mode)
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    out = np.zeros(4 * len(SITES))
    got = _probe_lib().oracle_ranges(bitrate, fs, pcm.ctypes.data, pcm.size, hop, out.ctypes.data)
    assert got == len(SITES), 'the probe knows %d sites' % got
    return {s: (int(r[0]), int(r[1]), int(r[2]), float(r[3])) for s, r in zip(SITES, out.reshape(-1, 4))}


def marg_max(mode, pcm):
    return ranges(mode, pcm)['sincos'][3]


# ------------------------------------------------------------------ the streams
@functools.lru_cache(maxsize=None)
def _synth(mode, n, lead=None):
    """the plain synthetic carrier of the mode (read-only: cached); lead: its zero lead-in"""
    bitrate, fs, _ = dims(mode)
    sec, f = n / fs + 0.01, CARRIER[mode]
    seed = SYNTH_SEED[bitrate]
    if bitrate == 10500:
        x = tl.synth(seconds=sec, seed=seed, carrier=f, ebn0=12.0, lead_in=1000 if lead is None else lead)
    elif bitrate == 8400:
        x = tl.synth_c(seconds=sec, seed=seed, carrier=f, ebn0=12.0, lead_in=1000 if lead is None else lead)
    else:
        x = tl.synth_msk(seconds=sec, bitrate=bitrate, baud=600, seed=seed, carrier=f, ebn0=12.0,
                         lead_in=500 if lead is None else lead, fs=fs)
    assert len(x) >= n
    x = x[:n]
    x.setflags(write=False)
    return x


def _noise(mode, n, salt=0, sigma=0.25 * 32768 / 3):
    rng = np.random.default_rng([SEED, dims(mode)[1], dims(mode)[0], salt])
    return np.clip(np.round(rng.normal(0, sigma, n)), -32768, 32767).astype(np.int16)


def _i16(x):
    return np.clip(x, -32768, 32767).astype(np.int16)


def _lock_hop(mode, pcm, frame=True):
    """(hops until the DataCarrierDetect rise, hops until that and a good
    frame and, C, a Call_progress SU) of pcm fed hop by hop; None: never"""
    bitrate, _, hop = dims(mode)
    o, rise = oracle(mode), None
    for k in range(len(pcm) // hop):
        o.push(pcm[k * hop:(k + 1) * hop])
        if rise is None and o.events()[0] >= 1:
            rise = k + 1
        if rise is not None and (not frame or (good_frames(o.frames()) >= 1 and
                                               (bitrate != 8400 or len(o.c_units()) >= 1))):
            return rise, k + 1
    return rise, None


@functools.lru_cache(maxsize=None)
def locking_stream(mode, name):
    """(stream, hops until the rise): a locking class at its searched length"""
    _, fs, hop = dims(mode)
    n = LOCK_HOPS_MAX * hop + TAIL
    if name == 'lead0':
        x = _synth(mode, n, lead=0)
    elif name == 'late':
        lead = late_lead(mode)
        x = _synth(mode, n, lead=lead).copy()
        x[:lead] = 0
    else:
        wide = _synth(mode, n).astype(np.int32)
        # (32768 has no int16: the negated stream is clipped)
        x = {'synth': wide, 'clip': wide * 8, 'tiny': wide // 2048, 'negated': -wide}[name]
        x = _i16(x)
    rise, stop = _lock_hop(mode, x, frame=mode not in NO_FRAME)
    assert stop is not None, '%s %s: the oracle does not lock within %d hops' % (mode, name, LOCK_HOPS_MAX)
    return x[:stop * hop + TAIL].copy(), rise


@functools.lru_cache(maxsize=None)
def cut_stream(mode, fill):
    """(stream, cut): the synthetic carrier cut off at the end of the hop after
    the one in which the oracle's DataCarrierDetect rises, continued with
    zeros ('silence'), +32767 ('fullscale') or noise, for as many whole hops
    as the ticked oracle's DataCarrierDetect takes to fall again (searched in
    steps of half a second; HOPS hops where it has not fallen within
    CUT_FALL_SECONDS)."""
    _, fs, hop = dims(mode)
    rise = locking_stream(mode, 'synth')[1]
    cut = (rise + 1) * hop
    longest = -(-(cut + CUT_FALL_SECONDS * fs) // hop) * hop + TAIL

    def make(n):
        y = np.zeros(n, dtype=np.int16)
        if fill == 'fullscale':
            y[:] = 32767
        elif fill == 'noise':
            y[:] = _noise(mode, longest, salt=1)[:n]
        y[:cut] = _synth(mode, LOCK_HOPS_MAX * hop + TAIL)[:cut]
        return y

    for half in range(1, 2 * CUT_FALL_SECONDS + 1):
        n = -(-(cut + half * fs // 2) // hop) * hop + TAIL
        if facts(mode, make(n), tick=True)['edges'] >= 2:
            return make(n), cut
    return make(cut + HOPS * hop + TAIL), cut


def _far_candidates(mode):
    """(label, stream) of the sincos search, lazily: full-scale tones and tones
    on a DC offset from FAR_STEP up to twice the locking bandwidth (the
    estimator's window before and after a hunter step) in steps of FAR_STEP,
    silent_hops + 6 hops long so that the hunter steps under them (OQPSK's
    rotation argument peaks in the last of those hops), and cut_fullscale with
    its cut moved"""
    _, fs, hop = dims(mode)
    n = (ci.silent_hops(mode) + HOPS) * hop + TAIL
    t = np.arange(n)
    step = FAR_STEP * fs / 48000
    for k in range(1, int(min(2 * ci.MODES[mode][4], fs / 2 - step) / step) + 1):
        f = k * step
        tone = np.cos(2 * np.pi * f / fs * t)
        yield 'tone %.3f Hz' % f, _i16(np.round(32767 * tone))
        yield 'tone %.3f Hz on DC' % f, _i16(np.round(16384 + 16383 * tone))
    cut0 = cut_stream(mode, 'fullscale')[1]
    syn = _synth(mode, LOCK_HOPS_MAX * hop + TAIL)
    for d in (-hop // 2, -hop // 4, 0, hop // 4, hop // 2):
        y = np.full(cut0 + (HOPS + 1) * hop + TAIL, 32767, dtype=np.int16)
        y[:cut0 + d] = syn[:cut0 + d]
        yield 'carrier cut into +32767 at %d' % (cut0 + d), y


@functools.lru_cache(maxsize=None)
def far_stream(mode):
    """(stream, label, its largest |marg.Val|, candidates tried): the first
    candidate whose rotation argument reaches aero_sincos_bf's bound (the
    search stops at the batch of FAR_BATCH that holds it), or, where none
    does, the one that comes closest"""
    _probe_lib()  # built and loaded before the threads start
    cands, tried, best = _far_candidates(mode), 0, None
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        while True:
            batch = list(itertools.islice(cands, FAR_BATCH))
            if not batch:
                break
            got = list(ex.map(lambda c: marg_max(mode, c[1]), batch))
            tried += len(batch)
            over = [k for k, m in enumerate(got) if m >= SINCOS_BOUND]
            k = over[0] if over else int(np.argmax(got))
            if over or best is None or got[k] > best[2]:
                best = batch[k][1], batch[k][0], got[k]
            if over:
                break
    return best + (tried,)


@functools.lru_cache(maxsize=None)
def streams(mode):
    """[(class, int16 stream)] in ORDER; the arrays are read-only."""
    bitrate, fs, hop = dims(mode)
    rng = np.random.default_rng([SEED, fs, bitrate])
    ns, n = ci.silent_hops(mode) * hop + TAIL, HOPS * hop + TAIL
    t = np.arange(n)
    out = {}
    out['silence'] = np.zeros(ns, dtype=np.int16)
    out['square'] = np.where((t // 3) % 2 == 0, 32767, -32768).astype(np.int16)
    out['const_min'] = np.full(n, -32768, dtype=np.int16)
    one = np.zeros(ns, dtype=np.int16)
    one[hop + hop // 2] = 29
    out['one_sample'] = one
    late = hop // 2 + agc_len(mode) + 2 * hop  # the first sample's FIR response has left the AGC ring
    two = np.zeros((late // hop + 3) * hop + TAIL, dtype=np.int16)
    two[hop // 2], two[late] = 32767, -32768
    out['two_samples'] = two
    out['lsb_noise'] = rng.integers(-1, 2, ns).astype(np.int16)
    out['noise'] = _noise(mode, n)
    out['tone'] = _i16(np.round(8000 * np.cos(2 * np.pi * CARRIER[mode] / fs * t)))
    out['tone_far'] = far_stream(mode)[0]
    for name in LOCKING:
        out[name] = locking_stream(mode, name)[0]
    for fill in ('silence', 'fullscale', 'noise'):
        out['cut_' + fill] = cut_stream(mode, fill)[0]
    syn = _synth(mode, LOCK_HOPS_MAX * hop + TAIL)[:n]
    period = max(2, round(1500 * fs / 48000))
    out['gated'] = np.where((t // period) % 2 == 0, syn, 0).astype(np.int16)
    wide = syn.astype(np.int32)
    out['overlap'] = _i16(wide + np.roll(wide, 7 * period // 3))
    assert set(out) == set(ORDER)
    for k, v in out.items():
        assert v.dtype == np.int16 and len(v) % hop == TAIL, k
        v.setflags(write=False)
    return [(name, out[name]) for name in ORDER]
