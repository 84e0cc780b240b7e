"""The Eb/N0 estimator of AERO_F_EBNO_MSK on the CPU: ebno.h's MSK step, walked
over an AGC ring and a ring of its own as the kernel walks them
(tools/hostcheck.cpp aero_x_ebno_msk_run), against a plain restatement of the
reference's MSKEbNoMeasure that keeps its own two 2 Fs-entry buffers
(tools/oracle_ebno_msk.cpp), by bit pattern.

The AGC ring is the oracle's own MSK AGC buffer (Fs entries), read after every
push: the walk sees what the kernel sees after a demod launch, never the
checker's buffers.  Streams, classes and cases: tests/ebno_msk_lib.py."""
import ctypes
import math
import os
import struct

import numpy as np
import pytest

import ebno_msk_lib as em

# which branches of the estimator each class takes (from the checker's own counts): all / some / none
# of its samples.  Every class but silence starts with 0 / 0 sums (its first sample follows zeros).
ALL, SOME, NONE = 'all', 'some', 'none'


@pytest.fixture(scope='module')
def hostcheck():
    so = os.environ.get('AERO_HOSTCHECK_SO')  # the sanitizer build (scripts/asan_check.sh)
    if not so:
        import build  # aero-cli_amd/build.py (aero_testlib puts it on the path)
        so = build.build_hostcheck()
    L = ctypes.CDLL(so)
    L.aero_x_ebno_msk_run.restype = ctypes.c_int
    L.aero_x_ebno_msk_run.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong,
                                      ctypes.c_longlong, ctypes.c_void_p]
    L.aero_x_ebno_msk_lg2.restype = ctypes.c_double
    L.aero_x_ebno_msk_lg2.argtypes = []
    return L


def _stops(a, b):
    """where the walk is read between samples a and b: every hop boundary (a channel stands there
    when (nsamp + 1) % HOP == 0) and the push end"""
    first = (a + 1 + em.HOP) // em.HOP * em.HOP - 1
    return [s for s in range(first, b, em.HOP)] + [b]


class Walker:
    """ebno.h's walk for one estimator (one rate): its state, its ring, its sample count"""

    def __init__(self, L, fs):
        self.L, self.fs = L, fs
        self.state = np.zeros(3)  # the model's start: zero sums, EbNo 0.0
        self.own = np.zeros(2 * fs)
        self.done = 0

    def after_push(self, o, n):
        """the oracle has just taken n more samples at this rate: [(local sample count, EbNo)] at every stop.
        A stop inside the push is walked from the ring the kernel would have seen then: the entries
        of the samples up to the stop are the same ones (the push is at most Fs samples)."""
        ring, ptr = o.agc_ring()
        a, b = self.done, self.done + n
        assert ptr == b % self.fs
        out = []
        for s in _stops(a, b):
            assert self.L.aero_x_ebno_msk_run(ring.ctypes.data, self.own.ctypes.data, self.fs, self.done, s,
                                              self.state.ctypes.data) == 0
            self.done = s
            out.append((s, self.state[2]))
        return out


def _compare(name, got, at, series):
    want = series[np.array(at) - 1]
    bad = np.flatnonzero(em.bits(got) != em.bits(want))
    assert bad.size == 0, '%s: EbNo differs after sample %d: %r, the checker %r' % (
        name, at[bad[0]], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize('name', em.CLASSES)
@pytest.mark.parametrize('case', sorted(em.CASES))
def test_walk_equals_checker_bitwise(hostcheck, case, name):
    bitrate, fs = em.CASES[case]
    o = em.EbnoMskOracle(bitrate, fs)
    x = em.stream(case, name)
    w = Walker(hostcheck, fs)
    got, at = [], []
    for a, b in em.messages(len(x), em.RAGGED):
        o.push(x[a:b])
        for s, v in w.after_push(o, b - a):
            at.append(s)
            got.append(v)
    series = o.series()
    assert len(series) == len(x) == em.n_of(case) and at[-1] == len(x)
    assert np.array_equal(em.bits(series), em.bits(em.reference(case, name)[0]))
    _compare('%s %s' % (case, name), got, at, series)
    assert not np.isnan(series).any() and series.max() <= 50.0  # (-inf, 50]


def test_rate_change_restarts_the_series(hostcheck):
    """30000 samples at 12 kHz, 24000 at 24 kHz, 30000 at 12 kHz: each leg is a fresh estimator
    (zero sums, ring and EbNo, the sample count from 0), the checker's re-created by the push."""
    o = em.EbnoMskOracle(600, em.RATE_LEGS[0][1])
    base, got, at = 0, [], []
    for x, fs in em.rate_stream():
        w = Walker(hostcheck, fs)
        for a, b in em.messages(len(x), em.RAGGED):
            o.push(x[a:b], fs)
            for s, v in w.after_push(o, b - a):
                at.append(base + s)
                got.append(v)
        base += len(x)
    series = o.series()
    assert len(series) == base == sum(n for n, _ in em.RATE_LEGS)
    _compare('rate change', got, at, series)
    assert np.array_equal(em.bits(series), em.bits(em.rate_reference()[0]))
    # a leg's first value is 0.8 * 0.0 + 0.2 * tebno of a one-sample window, whatever came before it:
    # the first and the third leg (both 12 kHz, different audio) start from the same state
    fresh = em.EbnoMskOracle(600, em.RATE_LEGS[2][1])
    x3 = em.rate_stream()[2][0]
    for a, b in em.messages(len(x3), em.RAGGED):
        fresh.push(x3[a:b])
    third = series[em.RATE_LEGS[0][0] + em.RATE_LEGS[1][0]:]
    # (the demodulator's own state carries over a rate change, so only the estimator's start is compared:
    # while the input is the lead-in's silence both are the NaN branch's 50 smoothed from 0.0)
    assert third[0] == fresh.series()[0] == 0.2 * 50


def test_walk_refuses_a_span_the_ring_does_not_hold(hostcheck):
    fs = 12000
    agc, own, state = np.zeros(fs), np.zeros(2 * fs), np.zeros(3)
    run = hostcheck.aero_x_ebno_msk_run
    assert run(agc.ctypes.data, own.ctypes.data, fs, 0, fs, state.ctypes.data) == 0
    assert run(agc.ctypes.data, own.ctypes.data, fs, fs, 2 * fs + 1, state.ctypes.data) == -1
    assert run(agc.ctypes.data, own.ctypes.data, fs, 5, 4, state.ctypes.data) == -1


def test_log10_of_two_has_glibcs_bits(hostcheck):
    assert struct.pack('<d', hostcheck.aero_x_ebno_msk_lg2()) == struct.pack('<d', math.log10(2.0))


EXPECT = {
    'silence': dict(nan=ALL, high=NONE, negarg=NONE, interior=NONE),
}


@pytest.mark.parametrize('case', sorted(em.CASES))
def test_branches_by_class(case):
    n = em.n_of(case)
    for name in em.CLASSES:
        br = em.reference(case, name)[1]
        print(case, name, br)
        # a sample takes the NaN branch, the clamp or neither (a NaN's 50 is not above 50);
        # a negative log argument is one way into the NaN branch
        assert br['nan'] + br['high'] + br['interior'] == n and br['negarg'] <= br['nan'], (name, br)
        for branch, how in EXPECT.get(name, {}).items():
            assert (br[branch] == n) if how == ALL else (br[branch] == 0), (name, br)
        if name != 'silence':
            assert 0 < br['nan'] < n and br['interior'] > 0, (name, br)


def test_classes_reach_the_nan_interior_and_negative_argument_branches():
    reached = {case: set() for case in em.CASES}
    for case in em.CASES:
        for name in em.CLASSES:
            reached[case] |= {b for b, k in em.reference(case, name)[1].items() if k}
    for case in em.CASES:
        assert {'nan', 'interior', 'negarg'} <= reached[case], case
    # a constant envelope (the full-scale DC of const_min at 12 kHz) crosses Var alpha^2 = 0.0085 on a
    # sample that takes the "> 50" clamp; no tone of the grid does (ebno_msk_lib)
    assert em.reference('600@12000', 'const_min')[1]['high'] >= 1


# ---- the step level: the "> 50" clamp, a zero mean and the -inf that stays, with hand-made inputs
# through aero_x_ebno_msk_run (fs = 4: a window of 8) against the checker's estimator alone.  No tone of
# the grid reaches the clamp in a whole stream ("The Eb/N0 estimate"; ebno_msk_lib.tone_search).
def _run_inputs(L, fs, inputs):
    """ebno.h's walk over hand-made estimator inputs, fs at a time through an AGC ring of fs entries"""
    x = np.ascontiguousarray(inputs, dtype=np.float64)
    agc, own, state = np.zeros(fs), np.zeros(2 * fs), np.zeros(3)
    out, done = [], 0
    while done < len(x):
        for k in range(done, min(done + fs, len(x))):
            agc[k % fs] = x[k]
            assert L.aero_x_ebno_msk_run(agc.ctypes.data, own.ctypes.data, fs, k, k + 1, state.ctypes.data) == 0
            out.append(state[2])
        done = min(done + fs, len(x))
    return np.array(out)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(em.bits(a), em.bits(b))


def test_step_takes_the_high_clamp(hostcheck):
    """a full window of 1 +- d has Mean 1 and Var d^2: Var alpha^2 - 0.0085 = 2 d^2 - 0.0085 lies in
    (0, 6.3e-6) for d just above sqrt(0.00425); and at exactly zero log10 gives -inf, tebno +inf -> 50"""
    fs, hits = 4, 0
    for d in np.sqrt(0.00425) + np.arange(1, 40) * 1e-6:
        x = np.tile([1.0 + d, 1.0 - d], 3 * fs)
        want, br = em.feed(2 * fs, x)
        assert _same(_run_inputs(hostcheck, fs, x), want), d
        hits += br['high']
    assert hits > 0


def test_step_zero_mean_and_the_infinity_that_stays(hostcheck):
    fs = 4
    # silence: Mean 0, alpha inf, Var alpha = 0 inf = NaN -> 50; then one huge sample whose square overflows
    # while the mean's does not (Mean = sig / 8): E2 = inf, Var = inf, log10(inf) = inf, tebno = -inf, and
    # EbNo = -inf for good (0.8 (-inf) + 0.2 t, t <= 50), also once the infinity has left the window
    # (inf - inf = NaN -> 50)
    x = np.array([0.0] * 5 + [5e154] + [0.25, 0.5] * 10)
    want, br = em.feed(2 * fs, x)
    got = _run_inputs(hostcheck, fs, x)
    assert _same(got, want)
    assert br['nan'] >= 5 and want[4] > 0 and np.all(np.isneginf(want[5:])) and np.all(np.isneginf(got[5:]))
    # a negative mean cannot come from fabs() inputs, but a residue of either sign can: what a cut
    # carrier leaves.  Sums of alternating large and tiny terms leave such residues
    y = np.array([1e16, 1.0, 1e-16, 3.0] * 2 + [0.0] * 12)
    want, br = em.feed(2 * fs, y)
    assert _same(_run_inputs(hostcheck, fs, y), want)


# ---- the flag, and the pool layout behind it (no GPU: the recorded layout, tests/test_channel_lifecycle_host.py)
def _plan(L, kind, flags, slot=0, C=64):
    n = L.aero_x_reset_plan(kind, C, flags, slot, None, 0)
    assert n > 0
    out = np.zeros(7 * n, dtype=np.uint64)
    assert L.aero_x_reset_plan(kind, C, flags, slot, out.ctypes.data_as(ctypes.c_void_p), n) == n
    return out.reshape(n, 7)


def _fingerprint(L, kind, flags):
    fp = ctypes.c_uint64()
    assert L.aero_x_plan_fingerprint(kind, 64, flags, ctypes.byref(fp)) == 0
    return fp.value


def test_flag_value_in_header_and_binding():
    import re

    import aero_engine as ae
    import aero_testlib as tl
    src = open(os.path.join(tl.ROOT, 'include', 'aero_engine.h')).read()
    assert re.search(r'#define AERO_F_EBNO_MSK 0x400\b', src)
    assert ae.F_EBNO_MSK == 0x400 and ae.F_EBNO == 0x200


# aero_x_reset_plan kinds: MSK 600 at 12 kHz, MSK 1200 at 24 kHz, MSK 600 at 48 kHz, generic 600 at 18750 Hz
MSK_KINDS = {1: 12000, 2: 24000, 4: 48000, 8 | (18750 << 8): 18750}


@pytest.mark.parametrize('kind', sorted(MSK_KINDS))
def test_the_ring_is_carved_only_with_the_flag(engine_lib, kind):
    import aero_engine as ae
    fs = MSK_KINDS[kind]
    L = engine_lib
    base, on = _plan(L, kind, 0), _plan(L, kind, ae.F_EBNO_MSK)
    # flag off, and AERO_F_EBNO alone: the layout every MSK pool had
    assert np.array_equal(_plan(L, kind, ae.F_EBNO), base)
    assert _fingerprint(L, kind, ae.F_EBNO) == _fingerprint(L, kind, 0) != _fingerprint(L, kind, ae.F_EBNO_MSK)
    # with it: the sums and EbNo [3][C], the done-count [C], the ring [2 Fs][C], behind what was there
    assert len(on) == len(base) + 3 and np.array_equal(on[:len(base)], base)
    rows = [(int(r[1]), int(r[2]), int(r[4])) for r in on[len(base):]]  # (bytes per row, rows, kind: 1 time-major)
    assert rows == [(8, 3, 1), (8, 1, 1), (8, 2 * fs, 1)]
    assert len(_plan(L, kind, ae.F_EBNO_MSK | ae.F_TRACE_HOPS)) == len(_plan(L, kind, ae.F_TRACE_HOPS)) + 5
    whole = lambda flags: int(_plan(L, kind, flags, slot=-1)[-1][0])  # the pool's size
    assert 16 * fs * 64 <= whole(ae.F_EBNO_MSK) - whole(0) < 16 * fs * 64 + 4 * 256 + 32 * 64


def test_other_kinds_are_laid_out_as_before(engine_lib):
    import aero_engine as ae
    for kind in (0, 10):  # OQPSK, C
        assert np.array_equal(_plan(engine_lib, kind, ae.F_EBNO_MSK), _plan(engine_lib, kind, 0))
        assert len(_plan(engine_lib, kind, ae.F_EBNO)) == len(_plan(engine_lib, kind, 0)) + 2


def test_steady_state_rises_with_the_carrier():
    """The estimate once the demodulator has held the carrier for longer than the window: the hop that
    ends 8 s into the stream.  (At 4.4 s the reference's MSK demodulator is still acquiring, its mse
    above the signal threshold, and the estimate near 0 whatever the carrier.)  The values are the
    reference's calibration, recorded in DESIGN.md; only their order is asserted."""
    for case in sorted(em.CASES):
        last = {k: em.steady(case, k) for k in (6, 10, 14)}
        print(case, {k: (v.min(), v.max()) for k, v in last.items()})
        assert last[6].max() < last[10].min() and last[10].max() < last[14].min(), case
