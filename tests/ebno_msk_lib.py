"""The checker of AERO_F_EBNO_MSK: the oracle plus a plain restatement of the
reference's MSKEbNoMeasure with its own two 2 Fs-entry buffers
(tools/liboracle_ebno_msk.so: oracle/aero_oracle.cpp as it stands and
tools/oracle_ebno_msk.cpp), and the streams the estimator is tested on.

A case is (AeroL bit rate, sample rate Fs); its streams are N = 4.4 Fs samples:
past the estimator's 2 Fs window, so the terms its moving averages drop are
live, and twice around the 2 Fs ring the engine keeps them in.  The classes are
those of tests/cont_inputs.py where they exist there (silence, one_sample,
square, const_min, lsb_noise, noise, gated, tone), the synthetic MSK carrier
(aero_testlib.synth_msk, 600 baud as a continuous MSK channel demodulates) at
6, 10 and 14 dB, and that carrier cut to digital silence after 2.5 s (`cut`:
the window drains but, in 4.4 s, never empties) and after 0.3 s (`cut_early`:
from 2.3 s on the sums are cancellation residues of either sign, as they are
behind `one_sample`).

The "> 50 dB" clamp.  A constant envelope a that fills the fraction f of the
window has Mean = f a and E2 = f a^2, so Var alpha^2 = 2 (1 - f) / f falls
through 0.0085 at f = 0.99577 (sample 23898 of 24000 at 12 kHz), and tebno
exceeds 50 only while the log's argument lies in [0, 6.3e-6): a band 3e-6 wide
in f, less than a tenth of a sample.  tone_search() looks for a tone of
cont_inputs' grid (15.625 Hz steps at 12 kHz, up to twice the locking
bandwidth) whose start-up transient puts a sample there.  None does, at any of
the three cases (115, 57 and 73 tones); of the classes only `const_min` at
12 kHz, a constant envelope too, lands one sample in the band.  So the clamp,
the -inf that stays and a zero mean are covered at the step level
(tests/test_ebno_msk_model.py)."""
import ctypes
import functools

import numpy as np

import aero_testlib as tl

HOP = 2048
SEED = 0xEB71
CASES = {'600@12000': (600, 12000), '1200@24000': (1200, 24000), '600@18750': (600, 18750)}
CARRIER = {600: 600.0, 1200: 1800.0}  # cont_inputs' MSK carriers
SYNTH_SEED = 21
CUT_SECONDS = 2.5
CUT_EARLY_SECONDS = 0.3  # the carrier has left the 2 s window by 2.3 s: 2.1 s of residue sums
RAGGED = (HOP - 1, HOP + 1, 3 * HOP + 7, 1, 2 * HOP - 8)  # 2047, 2049, 6151, 1, 4088
TONE_STEP = 62.5  # Hz at 48 kHz, scaled with Fs: cont_inputs.FAR_STEP
TONE_AMPLITUDE = 8000

# unlike neighbours side by side (silent, NaN lanes beside decoding ones)
CLASSES = ('silence', 'synth10', 'square', 'const_min', 'synth6', 'one_sample', 'lsb_noise', 'synth14', 'noise', 'cut',
           'tone', 'gated', 'cut_early')
BRANCHES = ('nan', 'high', 'negarg', 'interior')

# the rate-change stream: (samples, Fs) of each leg
RATE_LEGS = ((30000, 12000), (24000, 24000), (30000, 12000))


def n_of(case):
    return int(round(4.4 * CASES[case][1]))


def _so():
    import build  # aero-cli_amd/build.py (aero_testlib puts it on the path)
    return build.build_oracleebnomsk()


class EbnoMskOracle(tl.Oracle):
    """tl.Oracle over the hooked library; every push (at most Fs samples) feeds the estimator."""
    _libs = {}  # its own cache: tl.Oracle.lib() keeps the library under cls._libs['L']

    @classmethod
    def lib(cls):
        if 'L' not in cls._libs:
            saved = tl.ORACLE_SO
            tl.ORACLE_SO = _so()
            try:
                L = super().lib()
            finally:
                tl.ORACLE_SO = saved
            L.oracle_x_ebno_msk_update.argtypes = [ctypes.c_void_p]
            L.oracle_x_ebno_msk_update.restype = ctypes.c_longlong
            L.oracle_x_ebno_msk_series.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
            L.oracle_x_ebno_msk_series.restype = ctypes.c_size_t
            L.oracle_x_ebno_msk_branches.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            L.oracle_x_ebno_msk_branches.restype = None
            L.oracle_x_msk_agc_ring.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                ctypes.POINTER(ctypes.c_int)]
            L.oracle_x_msk_agc_ring.restype = ctypes.c_size_t
            L.oracle_x_ebno_msk_free.argtypes = [ctypes.c_void_p]
            L.oracle_x_ebno_msk_free.restype = None
            L.oracle_x_ebno_msk_feed.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t,
                                                 ctypes.c_void_p, ctypes.c_void_p]
            L.oracle_x_ebno_msk_feed.restype = None
        return cls._libs['L']

    def __init__(self, bitrate, fs):
        super().__init__(bitrate=bitrate)
        self.fs = fs
        self.pushed = 0

    def __del__(self):
        if getattr(self, 'h', None):
            self.L.oracle_x_ebno_msk_free(self.h)
        super().__del__()

    def push(self, pcm, fs=None):
        """one message at rate fs (default: the channel's last); a new rate re-creates the estimator"""
        if fs is not None:
            self.fs = fs
        assert len(pcm) <= self.fs
        super().push(pcm, self.fs)
        self.pushed += len(pcm)
        assert self.L.oracle_x_ebno_msk_update(self.h) == len(pcm)

    def series(self):
        """EbNo after every sample pushed"""
        return self._get(self.L.oracle_x_ebno_msk_series, np.float64)

    def branches(self):
        """{branch: times taken}: NaN -> 50, > 50, a negative log argument, neither clamp"""
        b = (ctypes.c_longlong * 4)()
        self.L.oracle_x_ebno_msk_branches(self.h, b)
        return dict(zip(BRANCHES, (int(v) for v in b)))

    def agc_ring(self):
        """(the AGC buffer of Fs entries, its pointer)"""
        ring = np.zeros(self.fs)
        ptr = ctypes.c_int()
        assert self.L.oracle_x_msk_agc_ring(self.h, ring.ctypes.data, ring.size, ctypes.byref(ptr)) == self.fs
        return ring, ptr.value


def feed(number, inputs, ebno0=0.0):
    """the checker's estimator alone, MSKEbNoMeasure(number), over hand-made inputs:
    (EbNo after every input, branch counts)"""
    L = EbnoMskOracle.lib()
    x = np.ascontiguousarray(inputs, dtype=np.float64)
    out = np.zeros(len(x))
    b = (ctypes.c_longlong * 4)()
    L.oracle_x_ebno_msk_feed(number, ebno0, x.ctypes.data, x.size, out.ctypes.data, b)
    return out, dict(zip(BRANCHES, (int(v) for v in b)))


def messages(n, sizes):
    """[start, stop) of the messages of an n-sample stream, their sizes cycled"""
    out, p, k = [], 0, 0
    while p < n:
        out.append((p, min(n, p + sizes[k % len(sizes)])))
        p = out[-1][1]
        k += 1
    return out


def _synth(bitrate, fs, n, ebn0):
    return tl.synth_msk(seconds=n / fs + 0.01, bitrate=bitrate, baud=600, seed=SYNTH_SEED, carrier=CARRIER[bitrate],
                        ebn0=float(ebn0), fs=fs)[:n]


def tone(fs, n, hz):
    return np.round(TONE_AMPLITUDE * np.cos(2 * np.pi * hz / fs * np.arange(n))).astype(np.int16)


@functools.lru_cache(maxsize=None)
def stream(case, name):
    """the int16 stream of a class (read-only: cached)"""
    bitrate, fs = CASES[case]
    n = n_of(case)
    rng = np.random.default_rng([SEED, fs, bitrate, len(name)] + [ord(ch) for ch in name])
    t = np.arange(n)
    if name == 'silence':
        x = np.zeros(n, dtype=np.int16)
    elif name == 'square':
        x = np.where((t // 3) % 2 == 0, 32767, -32768).astype(np.int16)
    elif name == 'const_min':
        x = np.full(n, -32768, dtype=np.int16)
    elif name == 'one_sample':
        x = np.zeros(n, dtype=np.int16)
        x[HOP + HOP // 2] = 29
    elif name == 'lsb_noise':
        x = rng.integers(-1, 2, n).astype(np.int16)
    elif name == 'noise':
        x = np.clip(np.round(rng.normal(0, 0.25 * 32768 / 3, n)), -32768, 32767).astype(np.int16)
    elif name == 'tone':
        x = tone(fs, n, CARRIER[bitrate])
    elif name in ('synth6', 'synth10', 'synth14'):
        x = _synth(bitrate, fs, n, name[5:])
    elif name in ('cut', 'cut_early'):
        x = stream(case, 'synth10').copy()
        x[int((CUT_SECONDS if name == 'cut' else CUT_EARLY_SECONDS) * fs):] = 0
    elif name == 'gated':
        period = max(2, round(1500 * fs / 48000))
        x = np.where((t // period) % 2 == 0, stream(case, 'synth10'), 0).astype(np.int16)
    else:
        raise KeyError(name)
    assert x.dtype == np.int16 and len(x) == n
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(case, name):
    """(EbNo after every sample, branch counts, hop records) of a class.  A continuous MSK channel's
    demodulation does not depend on the message boundaries, so one reference serves every schedule."""
    bitrate, fs = CASES[case]
    o = EbnoMskOracle(bitrate, fs)
    x = stream(case, name)
    for a, b in messages(len(x), RAGGED):
        o.push(x[a:b])
    s = o.series()
    s.setflags(write=False)
    return s, o.branches(), o.hops()


@functools.lru_cache(maxsize=None)
def rate_stream():
    """[(int16 audio, Fs)] of the rate-change stream: the 600-bps carrier synthesised at each leg's rate"""
    out = []
    for k, (n, fs) in enumerate(RATE_LEGS):
        x = tl.synth_msk(seconds=n / fs + 0.01, bitrate=600, baud=600, seed=SYNTH_SEED + k, carrier=CARRIER[600],
                         ebn0=10.0, fs=fs)[:n]
        x.setflags(write=False)
        out.append((x, fs))
    return out


@functools.lru_cache(maxsize=None)
def rate_reference():
    """(EbNo after every sample of the rate-change stream, hop records): the estimator re-created at each change"""
    o = EbnoMskOracle(600, RATE_LEGS[0][1])
    for x, fs in rate_stream():
        for a, b in messages(len(x), RAGGED):
            o.push(x[a:b], fs)
    s = o.series()
    s.setflags(write=False)
    return s, o.hops()


STEADY_SECONDS = 8


def steady(case, ebn0):
    """the checker's EbNo over the last hop of STEADY_SECONDS of the synthetic carrier at ebn0 dB"""
    bitrate, fs = CASES[case]
    n = STEADY_SECONDS * fs
    x = _synth(bitrate, fs, n, ebn0)
    o = EbnoMskOracle(bitrate, fs)
    for a, b in messages(n, (fs // 2,)):
        o.push(x[a:b])
    return o.series()[-HOP:]


def tone_search(case='600@12000', seconds=2.2):
    """{tone Hz: times the '> 50' clamp is taken} over cont_inputs' tone grid, by the checker; the
    clamp can only be met where the window is nearly full, so 2.2 s of each tone are enough"""
    bitrate, fs = CASES[case]
    step = TONE_STEP * fs / 48000
    n = int(seconds * fs)
    found = {}
    for k in range(1, int(min(2 * 900.0, fs / 2 - step) / step) + 1):
        o = EbnoMskOracle(bitrate, fs)
        x = tone(fs, n, k * step)
        for a, b in messages(n, (fs,)):
            o.push(x[a:b])
        found[k * step] = o.branches()['high']
    return found


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
