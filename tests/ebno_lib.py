"""The checker of AERO_F_EBNO: the oracle plus a plain restatement of the
reference's Eb/N0 estimator with its own two 96000-entry buffers
(tools/liboracle_ebno.so: oracle/aero_oracle.cpp as it stands and
tools/oracle_ebno.cpp), and the streams the estimator is tested on.

Streams are N = 201600 samples (4.2 s): past the estimator's 96000-sample
window, so the terms its moving averages drop are live, and past one wrap of
the 192000-entry AGC ring the engine reads them from.  The classes are those of
tests/cont_inputs.py where they exist there (silence, square, const_min,
one_sample, lsb_noise, noise, tone, gated), the synthetic P-channel carrier at
6, 10 and 14 dB, that carrier cut to silence after 2.5 s, and a C-channel
stream fed in 12000-sample messages.

`tone` is the class that reaches the estimator's "> 50 dB" clamp.  A constant
envelope a that fills the fraction f of the window has E = f a and E2 = f a^2,
so Var = a^2 f (1 - 1.024709 f) falls through zero near sample 93685, and mvr
exceeds 1e5 only while Var / Mean^2 < 3.1e-6: at most a sample or two, and
only where the filter's start-up transient lets a sample land there.  Found
with the checker on the tone grid of cont_inputs (62.5 Hz): 8062.5 Hz takes the
clamp 5 times (8000 Hz once, most others never)."""
import ctypes
import functools

import numpy as np

import aero_testlib as tl

N = 201600
HOP = 4096
WINDOW = 96000
AGC_LEN = 192000
SEED = 0xEB70
CARRIER = 8000.0
TONE_HZ = 8062.5
CUT_AT = 120000  # 2.5 s
C_MESSAGE = 12000

# OQPSK classes, unlike neighbours side by side (silent, NaN lanes beside decoding ones)
OQPSK = ('silence', 'synth10', 'square', 'const_min', 'synth6', 'one_sample', 'lsb_noise', 'synth14', 'noise', 'cut',
         'tone', 'gated')
BRANCHES = ('nan', 'high', 'low', 'floor', 'interior')

RAGGED = (HOP - 1, HOP + 1, 3 * HOP + 7, 1, 2 * HOP - 8)


def _so():
    import build  # aero-cli_amd/build.py (aero_testlib puts it on the path)
    return build.build_oracleebno()


class EbnoOracle(tl.Oracle):
    """tl.Oracle over the hooked library; every push (at most 96000 samples) feeds the estimator."""
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
            L.oracle_x_ebno_update.argtypes = [ctypes.c_void_p]
            L.oracle_x_ebno_update.restype = ctypes.c_longlong
            L.oracle_x_ebno_series.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
            L.oracle_x_ebno_series.restype = ctypes.c_size_t
            L.oracle_x_ebno_branches.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            L.oracle_x_ebno_branches.restype = None
            L.oracle_x_agc_ring.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.POINTER(ctypes.c_int)]
            L.oracle_x_agc_ring.restype = ctypes.c_size_t
            L.oracle_x_ebno_free.argtypes = [ctypes.c_void_p]
            L.oracle_x_ebno_free.restype = None
        return cls._libs['L']

    def __init__(self, bitrate=10500):
        super().__init__(bitrate=bitrate)
        self.pushed = 0

    def __del__(self):
        if getattr(self, 'h', None):
            self.L.oracle_x_ebno_free(self.h)
        super().__del__()

    def push(self, pcm, fs=None):
        assert len(pcm) <= WINDOW
        super().push(pcm, fs)
        self.pushed += len(pcm)
        assert self.L.oracle_x_ebno_update(self.h) == len(pcm)

    def series(self):
        """EbNo after every sample pushed"""
        return self._get(self.L.oracle_x_ebno_series, np.float64)

    def branches(self):
        """{branch: times taken}: NaN -> 50, > 50, < 0 -> 0, the 1e-9 floor, none of the first three"""
        b = (ctypes.c_longlong * 5)()
        self.L.oracle_x_ebno_branches(self.h, b)
        return dict(zip(BRANCHES, (int(v) for v in b)))

    def agc_ring(self):
        """(the AGC buffer, its pointer)"""
        ring = np.zeros(AGC_LEN)
        ptr = ctypes.c_int()
        assert self.L.oracle_x_agc_ring(self.h, ring.ctypes.data, ring.size, ctypes.byref(ptr)) == AGC_LEN
        return ring, ptr.value


def messages(n, sizes):
    """[start, stop) of the messages of an n-sample stream, their sizes cycled"""
    out, p, k = [], 0, 0
    while p < n:
        out.append((p, min(n, p + sizes[k % len(sizes)])))
        p = out[-1][1]
        k += 1
    return out


@functools.lru_cache(maxsize=None)
def stream(name):
    """the int16 stream of a class (read-only: cached); 'c' is the C-channel carrier"""
    rng = np.random.default_rng([SEED, len(name)] + [ord(ch) for ch in name])
    t = np.arange(N)
    if name == 'silence':
        x = np.zeros(N, dtype=np.int16)
    elif name == 'square':
        x = np.where((t // 3) % 2 == 0, 32767, -32768).astype(np.int16)
    elif name == 'const_min':
        x = np.full(N, -32768, dtype=np.int16)
    elif name == 'one_sample':
        x = np.zeros(N, dtype=np.int16)
        x[HOP + HOP // 2] = 29
    elif name == 'lsb_noise':
        x = rng.integers(-1, 2, N).astype(np.int16)
    elif name == 'noise':
        x = np.clip(np.round(rng.normal(0, 0.25 * 32768 / 3, N)), -32768, 32767).astype(np.int16)
    elif name == 'tone':
        x = np.round(8000 * np.cos(2 * np.pi * TONE_HZ / 48000 * t)).astype(np.int16)
    elif name in ('synth6', 'synth10', 'synth14'):
        x = tl.synth(seconds=N / 48000 + 0.01, seed=5, carrier=CARRIER, ebn0=float(name[5:]))[:N]
    elif name == 'cut':
        x = stream('synth10').copy()
        x[CUT_AT:] = 0
    elif name == 'gated':
        x = np.where((t // 1500) % 2 == 0, stream('synth10'), 0).astype(np.int16)
    elif name == 'c':
        x = tl.synth_c(seconds=N / 48000 + 0.01, seed=5, carrier=CARRIER, ebn0=12.0)[:N]
    else:
        raise KeyError(name)
    assert x.dtype == np.int16 and len(x) == N
    x.setflags(write=False)
    return x


def bitrate_of(name):
    return 8400 if name == 'c' else 10500


@functools.lru_cache(maxsize=None)
def reference(name, sizes=(C_MESSAGE,)):
    """(EbNo after every sample, branch counts, hop records) of a class fed in messages of `sizes`
    (cycled).  An OQPSK channel's demodulation does not depend on the message boundaries, so one
    reference serves every schedule; the C channel's does, and is fed as the tests feed it."""
    o = EbnoOracle(bitrate_of(name))
    x = stream(name)
    for a, b in messages(N, sizes):
        o.push(x[a:b])
    s = o.series()
    s.setflags(write=False)
    return s, o.branches(), o.hops()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
