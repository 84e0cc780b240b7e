"""The Eb/N0 estimator of AERO_F_EBNO on the CPU: ebno.h's step, walked over an
AGC ring as the kernel walks it (tools/hostcheck.cpp aero_x_ebno_run), against
a plain restatement of the reference's OQPSKEbNoMeasure that keeps its own two
96000-entry buffers (tools/oracle_ebno.cpp), by bit pattern.

The ring is the oracle's own AGC buffer, read after every push: the walk sees
what the kernel sees after a demod launch (the launch's samples in the ring,
the entries 96000 behind them not yet overwritten), never the checker's
buffers.  Streams and classes: tests/ebno_lib.py."""
import ctypes
import os

import numpy as np
import pytest

import ebno_lib as el

SCHEDULES = {'3000': (3000,), '12000': (12000,), '48000': (48000,), 'ragged': el.RAGGED}
C_SCHEDULES = ('3000', '12000')  # a C-channel message holds at most 32768 samples

# which branches of the estimator each class takes (from the checker's own counts): all / some / none
# of its samples.  Every class but silence starts with one 0 / 0 (its first sample follows zeros).
ALL, SOME, NONE = 'all', 'some', 'none'
EXPECT = {
    'silence': dict(nan=ALL, high=NONE, low=NONE, floor=NONE, interior=NONE),
    'one_sample': dict(nan=SOME, high=NONE, low=SOME, floor=SOME, interior=NONE),
    'square': dict(nan=SOME, high=NONE, low=SOME, floor=SOME, interior=SOME),
    'tone': dict(nan=SOME, high=SOME, low=SOME, floor=SOME, interior=SOME),
    'gated': dict(nan=SOME, high=NONE, low=SOME, floor=NONE, interior=NONE),
}
for _k in ('const_min', 'lsb_noise', 'noise', 'synth6', 'synth10', 'synth14', 'cut', 'c'):
    EXPECT[_k] = dict(nan=SOME, high=NONE, low=SOME, floor=NONE, interior=SOME)


@pytest.fixture(scope='module')
def hostcheck():
    so = os.environ.get('AERO_HOSTCHECK_SO')  # the sanitizer build (scripts/asan_check.sh)
    if not so:
        import build  # aero-cli_amd/build.py (aero_testlib puts it on the path)
        so = build.build_hostcheck()
    L = ctypes.CDLL(so)
    L.aero_x_ebno_run.restype = ctypes.c_int
    L.aero_x_ebno_run.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong,
                                  ctypes.c_double, ctypes.c_void_p]
    return L


def _stops(a, b):
    """where the walk is read between samples a and b: every hop boundary (a channel stands there
    when (nsamp + 1) % HOP == 0) and the message end"""
    first = (a + 1 + el.HOP) // el.HOP * el.HOP - 1
    return [s for s in range(first, b, el.HOP)] + [b]


def _walk_against_checker(L, name, sizes):
    o = el.EbnoOracle(el.bitrate_of(name))
    x = el.stream(name)
    fb = float(el.bitrate_of(name))
    state = np.zeros(3)  # the model's start: zero sums, EbNo 0.0
    done, got, at = 0, [], []
    for a, b in el.messages(el.N, sizes):
        o.push(x[a:b])
        ring, ptr = o.agc_ring()
        for s in _stops(a, b):
            # the pointer after sample s - 1: the ring's own, b - s samples back
            assert L.aero_x_ebno_run(ring.ctypes.data, el.AGC_LEN, (ptr - (b - s)) % el.AGC_LEN, done, s, fb,
                                     state.ctypes.data) == 0
            done = s
            got.append(state[2])
            at.append(s)
    series = o.series()
    assert len(series) == el.N and at[-1] == el.N
    want = series[np.array(at) - 1]
    bad = np.flatnonzero(el.bits(got) != el.bits(want))
    assert bad.size == 0, '%s: EbNo differs after sample %d: %r, the checker %r' % (
        name, at[bad[0]], got[bad[0]], want[bad[0]])
    return series, o.branches()


@pytest.mark.parametrize('name', el.OQPSK + ('c',))
def test_walk_equals_checker_bitwise(hostcheck, name):
    ref = None
    for sched in (C_SCHEDULES if name == 'c' else SCHEDULES):
        series, branches = _walk_against_checker(hostcheck, name, SCHEDULES[sched])
        if name != 'c':  # an OQPSK channel does not depend on its message boundaries
            if ref is None:
                ref = series
            assert np.array_equal(el.bits(series), el.bits(ref)), sched
    assert np.isfinite(series).all() and series.min() >= 0.0 and series.max() <= 50.0


def test_walk_refuses_a_span_the_ring_does_not_hold(hostcheck):
    ring, state = np.zeros(el.AGC_LEN), np.zeros(3)
    args = (ring.ctypes.data, el.AGC_LEN, 0)
    assert hostcheck.aero_x_ebno_run(*args, 0, el.AGC_LEN - el.WINDOW, 10500.0, state.ctypes.data) == 0
    assert hostcheck.aero_x_ebno_run(*args, 0, el.AGC_LEN - el.WINDOW + 1, 10500.0, state.ctypes.data) == -1
    assert hostcheck.aero_x_ebno_run(*args, 5, 4, 10500.0, state.ctypes.data) == -1


@pytest.mark.parametrize('name', sorted(EXPECT))
def test_branches_by_class(name):
    br = el.reference(name)[1]
    for branch, how in EXPECT[name].items():
        n = br[branch]
        if how == ALL:
            assert n == el.N, (name, br)
        elif how == SOME:
            assert 0 < n < el.N, (name, br)
        else:
            assert n == 0, (name, br)
    # interior is "none of the three clamps"; the floor always ends in the < 0 clamp
    assert br['nan'] + br['high'] + br['low'] + br['interior'] == el.N and br['floor'] <= br['low']


def test_classes_reach_every_branch():
    reached = set()
    for name in EXPECT:
        reached |= {b for b, n in el.reference(name)[1].items() if n}
    assert reached == set(el.BRANCHES)


def test_steady_state_rises_with_the_carrier():
    """The estimate once the window holds carrier only (the last hop of the stream).  The values are
    the reference's calibration, recorded in DESIGN.md; only their order is asserted."""
    last = {k: el.reference('synth%d' % k)[0][-el.HOP:] for k in (6, 10, 14)}
    print({k: (v.min(), v.max()) for k, v in last.items()})
    assert last[6].max() < last[10].min() and last[10].max() < last[14].min()
