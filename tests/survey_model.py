"""The wideband carrier survey restated in numpy (include/aero_chan.h
"Wideband carrier survey"): the checker of aero-cli_amd/csrc/survey.hip and
of aero_survey_peaks.

SurveyModel follows the contract line by line: float32 -> float64, the window
product, the oracle's JFFT (oracle_fft) per segment, re*re + im*im, and one
sequential acc = acc + p per segment, with the unfinished tail carried from
one feed() to the next.  numpy evaluates every elementwise operation on its
own, so nothing is contracted.  dc_remove is demodData's DC removal
(publish/publisher.cpp:292-296) in float32 scalars.  peaks() restates
aero_survey_peaks in Python floats, operation by operation."""
import functools
import math

import numpy as np

import aero_testlib as tl

B288 = 57600  # complex samples per read at 288 ksps


def hann(n):
    """0.5 - 0.5 cos(2 pi i / N) as aero_engine.Channeliser.survey_start('hann') builds it"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def odd_window(n):
    """exact small multiples of 1/4 with zeros and negative values"""
    i = np.arange(n)
    return ((i * 37) % 11 - 5) / 4.0


WINDOWS = {'none': lambda n: None, 'hann': hann, 'odd': odd_window}


def dc_remove(x, state=None):
    """avept = avept*(1 - 1e-6) + 1e-6*x; x -= avept per arm, in float32 as
    dc_kernel evaluates it.  x: complex64; state: [re, im] float32 carried
    between calls (changed in place).  Returns the corrected complex64 copy."""
    if state is None:
        state = [np.float32(0), np.float32(0)]
    k1 = np.float32(1.0) - np.float32(0.000001)
    k2 = np.float32(0.000001)
    out = np.array(x, dtype=np.complex64)
    v = out.view(np.float32)
    for arm in (0, 1):
        a = np.float32(state[arm])
        col = v[arm::2].copy()
        for i in range(len(col)):
            c = col[i]
            a = a * k1 + k2 * c
            col[i] = c - a
        v[arm::2] = col
        state[arm] = a
    return out


def segment_power(seg, window):
    """p[k] of one segment of complex64 samples"""
    n = len(seg)
    re, im = seg.real.astype(np.float64), seg.imag.astype(np.float64)
    if window is not None:
        re, im = re * window, im * window
    buf = np.empty(2 * n, dtype=np.float64)
    buf[0::2], buf[1::2] = re, im
    tl.Oracle.lib().oracle_fft(buf.ctypes.data, n, 0)
    xr, xi = buf[0::2], buf[1::2]
    return xr * xr + xi * xi


class SurveyModel:
    def __init__(self, log2n, window=None):
        self.n = 1 << log2n
        self.window = None if window is None else np.asarray(window, dtype=np.float64)
        self.acc = np.zeros(self.n, dtype=np.float64)
        self.segments = 0
        self.total = 0  # segments since the start
        self.carry = np.zeros(0, dtype=np.complex64)

    def feed(self, x):
        """the next samples of the stream (complex64, any number)"""
        s = np.concatenate([self.carry, np.asarray(x, dtype=np.complex64)])
        nseg = len(s) // self.n
        for k in range(nseg):
            self.acc = self.acc + segment_power(s[k * self.n:(k + 1) * self.n], self.window)
        self.segments += nseg
        self.total += nseg
        self.carry = s[nseg * self.n:].copy()

    def read(self, reset=False):
        out = (self.acc.copy(), self.segments)
        if reset:
            self.acc = np.zeros(self.n, dtype=np.float64)
            self.segments = 0
        return out


def survey(x, log2n, window=None):
    """(acc, segments) of the whole stream x"""
    m = SurveyModel(log2n, window)
    m.feed(x)
    return m.read()


# ---------------------------------------------------------------- inputs
TONES3 = [(21500.0, 0.3), (-49000.0, 0.03), (91000.0, 0.1)]  # three levels, 288 ksps


@functools.lru_cache(maxsize=None)
def stream(kind, fs=288000, nreads=7, block=B288):
    """The input classes of tests/test_gpu_survey.py; computed once, not to be changed."""
    n = nreads * block
    if kind == 'tones':
        x = tl.wideband(fs, n, 0x5EE + nreads, TONES3 if fs == 288000 else [(f * fs / 288000.0, a) for f, a in TONES3])
    elif kind == 'zeros':
        x = np.zeros(n, dtype=np.complex64)
    elif kind == 'fullscale':
        rng = np.random.default_rng(0xF5)
        x = (rng.choice([-1.0, 1.0], n) + 1j * rng.choice([-1.0, 1.0], n)).astype(np.complex64)
    elif kind == 'tailpulse':  # one nonzero sample in the tail every segment size carries out of read 1
        x = np.zeros(n, dtype=np.complex64)
        x[2 * block - 5] = 0.75 - 0.5j
    elif kind == 'dc':
        x = (tl.wideband(fs, n, 0xDC, TONES3) + np.complex64(0.125 - 0.0625j)).astype(np.complex64)
    else:
        raise ValueError(kind)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(kind, log2n, window='none', fs=288000, nreads=7, block=B288, dcc=False):
    """(acc, segments) of stream(kind, ...), survey started before the first read"""
    x = stream(kind, fs, nreads, block)
    if dcc:
        x = dc_remove(x)
    acc, seg = survey(x, log2n, WINDOWS[window](1 << log2n))
    acc.setflags(write=False)
    return acc, seg


# ---------------------------------------------------------------- aero_survey_peaks
def llround(x):
    """C's llround: half away from zero (x - trunc(x) is exact)"""
    t = math.trunc(x)
    if abs(x - t) >= 0.5:
        t += 1 if x > 0 else -1
    return t


def fdiv(a, b):
    """IEEE division where Python raises"""
    if b == 0.0:
        return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a)
    return a / b


def peaks(power, log2n, sample_rate, center, mix_offset=0, threshold=8.0, min_bins=2, merge_gap=2):
    """aero_survey_peaks step by step; every float operation is one IEEE double operation"""
    n = 1 << log2n
    h = n // 2
    p = [float(v) for v in power]
    assert len(p) == n
    q = [p[(i + h) % n] for i in range(n)]
    floor = sorted(q)[(n - 1) // 2]
    limit = threshold * floor
    runs = []
    i = 0
    while i < n:
        if not q[i] > limit:
            i += 1
            continue
        b = i
        while b + 1 < n and q[b + 1] > limit:
            b += 1
        if runs and i - runs[-1][1] - 1 <= merge_gap:
            runs[-1][1] = b
        else:
            runs.append([i, b])
        i = b + 1
    fs, dn = float(sample_rate), float(n)
    out = []
    for a, b in runs:
        w = b - a + 1
        if w < min_bins:
            continue
        tot = num = den = 0.0
        for i in range(a, b + 1):
            f = float(i - h) * fs / dn
            e = q[i] - floor
            tot = tot + q[i]
            num = num + e * f
            den = den + e
        off = num / den if den > 0 else (float(a - h) * fs / dn + float(b - h) * fs / dn) / 2.0
        out.append(dict(offset_hz=off, bandwidth_hz=float(w) * fs / dn, ratio=fdiv(tot / float(w), floor),
                        frequency=center + llround(off) - mix_offset, first_bin=a, last_bin=b))
    return out
