"""The hold's model (tests/survey_hold_model.py) on the stream `gated`: what the
averaged spectrum misses and the peak spectrum finds; and the C
aero_survey_activity against its Python restatement, bit for bit.  No GPU: the
engine library loads on a CPU-only host."""
import math
import struct

import numpy as np
import pytest

import survey_hold_model as hm
import survey_model as sm

FS, C = 288000, 1545000000
TH = 8.0


def bits(v):
    return struct.pack('<d', v)


def same(got, want, what=''):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        for key in ('on_ratio', 'off_ratio', 'duty'):
            # a NaN's sign and payload are the processor's choice (0 / 0 is a negative NaN on x86)
            ok = math.isnan(g[key]) if math.isnan(w[key]) else bits(g[key]) == bits(w[key])
            assert ok, '%s: %s %r != %r' % (what, key, g[key], w[key])
        assert g['kind'] == w['kind'], what


def test_gated_carrier_is_found_on_the_peak_spectrum_only(cpu_libs):
    """log2n 12, Hann, group 4, level 8 * 4 * floor / segments, gated amplitude 0.008 (the
    recipe's; not raised).  Measured with the oracle's FFT: 98 segments, 24 groups.
    The averaged sums give two carriers (-49000 Hz, ratio 247.0; +21500 Hz, ratio 14759.2), the
    peak spectrum three: the third at +60004.4 Hz, bins 2901..2902, ratio 14.58.  Activity of the
    three runs (on / off / duty): -49 kHz 265.2 / 225.3 / 1.0, +21.5 kHz 14872.1 / 14637.1 / 1.0,
    +60 kHz 31.45 / 0.258 / 0.1667 (CONTINUOUS, CONTINUOUS, BURST).  The largest peak of a bin
    more than 3 bins away from a run is 4.962 times the group floor (the level is 8 times), so
    none of them is ever busy."""
    r = hm.gated_reference(12, 4)
    assert r['segments'] == 98 and r['groups'] == 24
    avg = sm.peaks(r['acc'], 12, FS, C, threshold=TH)
    assert len(avg) == 2
    for p, (tone, _) in zip(avg, sorted(hm.GATED_TONES)):
        assert abs(p['offset_hz'] - tone) <= FS / 4096
    found = sm.peaks(r['peak'], 12, FS, C, threshold=TH)
    print('averaged', avg, 'peak', found)
    assert len(found) == 3
    gp = found[2]
    assert abs(gp['offset_hz'] - hm.GATED_HZ) <= FS / 4096
    assert [abs(p['offset_hz'] - q['offset_hz']) <= FS / 4096 for p, q in zip(found, avg)] == [True, True]
    act = hm.activity(r['acc'], r['segments'], r['peak'], r['low'], r['busy'], r['groups'], 4, 12, TH, found)
    print('activity', act)
    assert [a['kind'] for a in act] == [hm.CONTINUOUS, hm.CONTINUOUS, hm.BURST]
    assert 0.0 < act[2]['duty'] < 0.5
    far = np.ones(4096, dtype=bool)
    for p in found:
        for i in range(p['first_bin'] - 3, p['last_bin'] + 4):
            far[(i + 2048) % 4096] = False
    fgrp = hm.lower_median(r['acc']) / r['segments'] * 4
    print('largest noise bin %.3f x the group floor' % (r['peak'][far].max() / fgrp))
    assert not r['busy'][far].any()
    assert r['busy'][~far].any()


def _c_activity(*a):
    import aero_engine as ae
    return ae.survey_activity(*a)


@pytest.mark.parametrize('log2n,group', [(12, 4), (13, 3), (14, 2)])
def test_activity_on_the_models_arrays(engine_lib, cpu_libs, log2n, group):
    r = hm.gated_reference(log2n, group)
    runs = sm.peaks(r['peak'], log2n, FS, C, threshold=TH)
    assert len(runs) >= 2
    n = 1 << log2n
    # and runs nobody found: the band's two ends, one bin, all of it
    runs = runs + [dict(first_bin=0, last_bin=5), dict(first_bin=n - 3, last_bin=n - 1), dict(first_bin=0, last_bin=0),
                   dict(first_bin=n - 1, last_bin=n - 1), dict(first_bin=n // 2, last_bin=n // 2),
                   dict(first_bin=0, last_bin=n - 1)]
    args = (r['acc'], r['segments'], r['peak'], r['low'], r['busy'], r['groups'], group, log2n, TH, runs)
    want = hm.activity(*args)
    same(_c_activity(*args), want, 'with busy')
    assert {w['kind'] for w in want} == {hm.IDLE, hm.CONTINUOUS, hm.BURST} or log2n != 12
    args = args[:4] + (None,) + args[5:]
    want = hm.activity(*args)
    assert all(w['duty'] == -1.0 for w in want)
    same(_c_activity(*args), want, 'busy NULL')
    # a smaller threshold and other counts: other kinds
    args = (r['acc'], 3, r['peak'], r['low'], r['busy'], 7, group + 1, log2n, 0.25, runs)
    same(_c_activity(*args), hm.activity(*args), 'other counts')


def test_activity_over_a_zero_floor(engine_lib):
    """an all-zero spectrum: fgrp is 0, a zero sum gives NaN (kind IDLE), a positive one +infinity"""
    n = 16
    runs = [dict(first_bin=0, last_bin=1), dict(first_bin=8, last_bin=8), dict(first_bin=14, last_bin=15)]
    power, peak, low = np.zeros(n), np.zeros(n), np.zeros(n)
    busy = np.zeros(n, dtype=np.uint32)
    peak[0] = 2.0  # ascending index 8
    peak[6], low[6], busy[6] = 3.0, 1.0, 5  # ascending index 14
    args = (power, 4, peak, low, busy, 9, 2, 4, TH, runs)
    want = hm.activity(*args)
    assert math.isnan(want[0]['on_ratio']) and want[0]['kind'] == hm.IDLE
    assert want[1]['on_ratio'] == math.inf and math.isnan(want[1]['off_ratio']) and want[1]['kind'] == hm.BURST
    assert want[2]['off_ratio'] == math.inf and want[2]['kind'] == hm.CONTINUOUS
    same(_c_activity(*args), want, 'zero floor')


def test_activity_with_low_still_infinite(engine_lib):
    """a hold that was read before its first group: off_ratio is +infinity"""
    n = 64
    rng = np.random.default_rng(5)
    power, peak = rng.uniform(1, 2, n), rng.uniform(1, 40, n)
    low = np.full(n, np.inf)
    runs = [dict(first_bin=3, last_bin=9), dict(first_bin=63, last_bin=63)]
    args = (power, 10, peak, low, np.zeros(n, dtype=np.uint32), 1, 3, 6, 2.0, runs)
    want = hm.activity(*args)
    assert all(w['off_ratio'] == math.inf for w in want)
    same(_c_activity(*args), want, 'low +inf')


def test_activity_invalid(engine_lib):
    import aero_engine as ae
    n = 16
    good = dict(power=np.ones(n), segments=4, peak=np.ones(n), low=np.ones(n), busy=np.zeros(n, dtype=np.uint32),
                groups=2, group=2, log2n=4, threshold=8.0, runs=[dict(first_bin=1, last_bin=2)])
    order = ('power', 'segments', 'peak', 'low', 'busy', 'groups', 'group', 'log2n', 'threshold', 'runs')

    def both(**kw):
        a = dict(good, **kw)
        args = tuple(a[k] for k in order)
        with pytest.raises(ValueError):
            hm.activity(*args)
        with pytest.raises(ae.AeroError) as e:
            ae.survey_activity(*args)
        assert e.value.rc == ae.AERO_E_INVALID

    same(ae.survey_activity(*(good[k] for k in order)), hm.activity(*(good[k] for k in order)), 'valid')

    def with_value(v, at=5):
        a = np.ones(n)
        a[at] = v
        return a

    both(segments=0)
    both(groups=0)
    both(group=0)
    both(group=-1)
    both(threshold=0.0)
    both(threshold=-1.0)
    both(threshold=math.nan)
    for bad in (-1.0, math.nan, math.inf, -math.inf):
        both(power=with_value(bad))
        both(peak=with_value(bad, n - 1))
    for a, b in ((-1, 2), (3, n), (5, 4), (n, n)):
        both(runs=[dict(first_bin=1, last_bin=2), dict(first_bin=a, last_bin=b)])
    for log2n in (1, 25, 0, -3):  # checked before any array is read
        both(log2n=log2n)
