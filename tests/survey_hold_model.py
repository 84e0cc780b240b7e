"""The survey's peak / min hold restated in numpy (include/aero_chan.h "Peak /
min hold, duty and a waterfall"): the checker of survey_hold_kernel
(aero-cli_amd/csrc/survey.hip) and of aero_survey_activity.

HoldModel follows the contract line by line on the segment powers of
survey_model.segment_power (the oracle's JFFT): gsum = gsum + p per segment,
and after the group's last segment the three comparisons, the ring row and
gsum = +0.  SurveyHoldModel is survey_model.SurveyModel with such a hold
beside it, fed from the same segments.  activity() restates
aero_survey_activity in Python floats, operation by operation."""
import functools
import math

import numpy as np

import aero_testlib as tl
import survey_model as sm

IDLE, CONTINUOUS, BURST = 0, 1, 2


class HoldModel:
    def __init__(self, n, group, rows=0, level=None):
        self.n, self.group, self.rows = n, group, rows
        self.level = None if level is None else np.array(level, dtype=np.float64)
        self.gsum = np.zeros(n)
        self.fill = 0
        self.gidx = 0  # groups since the start
        self.ring = {}  # group index -> sums, the last `rows` of them
        self._reset()

    def _reset(self):
        self.peak = np.zeros(self.n)
        self.low = np.full(self.n, np.inf)
        self.busy = np.zeros(self.n, dtype=np.uint32)
        self.groups = 0

    def segment(self, p):
        """the next completed segment's power"""
        self.gsum = self.gsum + p
        self.fill += 1
        if self.fill < self.group:
            return
        s = self.gsum
        with np.errstate(invalid='ignore'):
            self.peak = np.where(s > self.peak, s, self.peak)
            self.low = np.where(s < self.low, s, self.low)
            if self.level is not None:
                self.busy = self.busy + (np.isfinite(self.level) & (s > self.level)).astype(np.uint32)
        if self.rows:
            self.ring[self.gidx] = s.copy()
            self.ring.pop(self.gidx - self.rows, None)
        self.gsum = np.zeros(self.n)
        self.fill = 0
        self.gidx += 1
        self.groups += 1

    def read(self, reset=False):
        out = (self.peak.copy(), self.low.copy(), self.busy.copy(), self.groups)
        if reset:
            self._reset()
        return out

    def read_rows(self, cap_rows=None):
        """(rows[n][N] oldest first, first_group, whether cap_rows was too small)"""
        keys = sorted(self.ring)
        full = cap_rows is not None and cap_rows < len(keys)
        if full:
            keys = keys[len(keys) - cap_rows:]
        rows = np.array([self.ring[g] for g in keys], dtype=np.float64).reshape(len(keys), self.n)
        return rows, (keys[0] if keys else self.gidx), full


class SurveyHoldModel(sm.SurveyModel):
    """SurveyModel whose segments also go to self.hold while one is set"""

    def __init__(self, log2n, window=None):
        super().__init__(log2n, window)
        self.hold = None

    def hold_start(self, group, rows=0, level=None):
        self.hold = HoldModel(self.n, group, rows, level)

    def feed(self, x):
        s = np.concatenate([self.carry, np.asarray(x, dtype=np.complex64)])
        nseg = len(s) // self.n
        for k in range(nseg):
            p = sm.segment_power(s[k * self.n:(k + 1) * self.n], self.window)
            self.acc = self.acc + p
            if self.hold is not None:
                self.hold.segment(p)
        self.segments += nseg
        self.total += nseg
        self.carry = s[nseg * self.n:].copy()


# ---------------------------------------------------------------- inputs
GATED_TONES = [(21500.0, 0.3), (-49000.0, 0.03)]  # continuous
GATED_HZ, GATED_AMP = 60000.0, 0.008
GATES = ((2.2, 2.8), (5.1, 5.7))  # in reads


@functools.lru_cache(maxsize=None)
def gated(amp=GATED_AMP):
    """7 reads at 288 ksps: noise of sigma 0.05 drawn as aero_testlib.wideband draws it, two
    continuous tones and one at +60 kHz that is on during two stretches of 0.6 reads: about 17 %
    of the time.  Computed once, not to be changed."""
    fs, n, b = 288000, 7 * sm.B288, sm.B288
    rng = np.random.default_rng(0xB057)
    x = (rng.normal(0, 0.05, n) + 1j * rng.normal(0, 0.05, n)).astype(np.complex128)
    t = np.arange(n) / float(fs)
    for f, a in GATED_TONES:
        x += a * np.exp(2j * np.pi * f * t)
    for lo, hi in GATES:
        i, j = int(lo * b), int(hi * b)
        x[i:j] += amp * np.exp(2j * np.pi * GATED_HZ * t[i:j])
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


def stream(kind, **kw):
    """'gated', or an input class of survey_model.stream"""
    return gated() if kind == 'gated' else sm.stream(kind, **kw)


def lower_median(power):
    return sorted(float(v) for v in power)[(len(power) - 1) // 2]


def model_level(acc, segments, group, threshold=8.0):
    """threshold * group * floor / segments in every bin: what a group sum of the floor's bins
    would have to exceed threshold times"""
    return np.full(len(acc), threshold * group * lower_median(acc) / segments)


def run_model(x, log2n, group, rows=0, level=None, window=None, block=sm.B288):
    """the whole stream x read by read, survey and hold started before the first read"""
    m = SurveyHoldModel(log2n, window)
    m.hold_start(group, rows, level)
    for b in range(0, len(x), block):
        m.feed(x[b:b + block])
    return m


@functools.lru_cache(maxsize=None)
def gated_reference(log2n, group, rows=0, window='hann', threshold=8.0):
    """The model on `gated` with the level of model_level: a dict with acc, segments, level, peak,
    low, busy, groups, rows and first_group; read-only."""
    x = gated()
    w = sm.WINDOWS[window](1 << log2n)
    acc, seg = sm.survey(x, log2n, w)
    level = model_level(acc, seg, group, threshold)
    m = run_model(x, log2n, group, rows, level, w)
    peak, low, busy, groups = m.hold.read()
    ring, first, _ = m.hold.read_rows()
    out = dict(acc=m.acc, segments=m.segments, level=level, peak=peak, low=low, busy=busy, groups=groups, rows=ring,
               first_group=first)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---------------------------------------------------------------- aero_survey_activity
def activity(power, segments, peak, low, busy, groups, group, log2n, threshold, runs):
    """aero_survey_activity step by step; every float operation is one IEEE double operation.
    ValueError where the C function returns AERO_E_INVALID."""
    if segments == 0 or groups == 0 or group < 1 or log2n < 2 or log2n > 24 or not threshold > 0:
        raise ValueError('invalid')
    n = 1 << log2n
    h = n // 2
    power, peak, low = ([float(v) for v in a] for a in (power, peak, low))
    for v in power + peak:
        if not v >= 0 or v == math.inf:
            raise ValueError('invalid')
    for r in runs:
        if r['first_bin'] < 0 or r['last_bin'] >= n or r['first_bin'] > r['last_bin']:
            raise ValueError('invalid')
    floor = sorted(power)[(n - 1) // 2]
    fgrp = floor / float(segments) * float(group)
    out = []
    for r in runs:
        a, b = r['first_bin'], r['last_bin']
        w = b - a + 1
        on = off = 0.0
        nb = 0
        for i in range(a, b + 1):
            k = (i + h) % n
            on = on + peak[k]
            off = off + low[k]
            if busy is not None:
                nb += int(busy[k])
        on_ratio = sm.fdiv(on / float(w), fgrp)
        off_ratio = sm.fdiv(off / float(w), fgrp)
        duty = float(nb) / (float(w) * float(groups)) if busy is not None else -1.0
        kind = IDLE if not on_ratio > threshold else CONTINUOUS if off_ratio > threshold else BURST
        out.append(dict(on_ratio=on_ratio, off_ratio=off_ratio, duty=duty, kind=kind))
    return out
