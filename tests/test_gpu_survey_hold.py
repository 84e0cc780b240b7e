"""The survey's peak / min hold (survey_hold_kernel in aero-cli_amd/csrc/survey.hip,
aero_chan_survey_hold_* in include/aero_chan.h) against its numpy restatement
(tests/survey_hold_model.py, on the oracle's JFFT).  Every comparison is of bit
patterns; no tolerance.  288 ksps, reads of 57600 samples: 14.06, 7.03 and 3.52
segments per read, so groups of 4, 3 and 2 segments straddle the runs."""
import functools

import numpy as np
import pytest

import aero_testlib as tl
import survey_hold_model as hm
import survey_model as sm

pytestmark = pytest.mark.gpu

C = tl.CENTER
CFG = tl.PUB_CONFIGS['r288k']
FS = CFG['sample_rate']
B = sm.B288


def chan(max_blocks=1, host_out=False, dcc=False, cfg=CFG):
    import aero_engine as ae
    return ae.Channeliser(cfg['sample_rate'], C, cfg['mains'], cfg['vfos'], correct_dc_bias=dcc, max_blocks=max_blocks,
                          host_out=host_out)


def reads(x, block=B):
    return [x[b * block:(b + 1) * block] for b in range(len(x) // block)]


def one_read_per_run(ch, x, block=B):
    for r in reads(x, block):
        ch.push(r)
        ch.run()


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, '%s: %r %s, the model has %r %s' % (
        what, got.shape, got.dtype, want.shape, want.dtype)
    view = np.uint64 if got.dtype == np.float64 else np.uint32
    bad = np.flatnonzero(got.view(view).ravel() != want.view(view).ravel())
    assert bad.size == 0, '%s: %d of %d values differ, first %d: %r != %r' % (
        what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def hold_equal(got, want, what=''):
    """(peak, low, busy, groups) of survey_hold_read and of HoldModel.read"""
    assert got[3] == want[3], '%s: %d groups, the model has %d' % (what, got[3], want[3])
    for g, w, name in zip(got[:3], want[:3], ('peak', 'low', 'busy')):
        same_bits(g, w, '%s: %s' % (what, name))


def rows_equal(got, want, what=''):
    """(rows, first_group) of survey_hold_rows and of HoldModel.read_rows"""
    assert got[1] == want[1], '%s: first group %d, the model has %d' % (what, got[1], want[1])
    same_bits(got[0], want[0], what + ': rows')


def survey_equal(got, want, what=''):
    assert got[1] == want[1], '%s: %d segments, the model has %d' % (what, got[1], want[1])
    same_bits(got[0], want[0], what + ': survey sums')


def all_equal(ch, m, what, cap_rows=None):
    """survey sums, hold and, where it has one, the ring of the channeliser against the model m"""
    survey_equal(ch.survey_read(), m.read(), what)
    hold_equal(ch.survey_hold_read(), m.hold.read(), what)
    if m.hold.rows:
        rows_equal(ch.survey_hold_rows(), m.hold.read_rows()[:2], what)


@functools.lru_cache(maxsize=None)
def gated_model(log2n, group, rows=5, max_reads=7):
    """the model after the first max_reads reads of `gated`, Hann window, the model's level of
    the whole stream; shared, not to be changed"""
    r = hm.gated_reference(log2n, group)
    return hm.run_model(hm.gated()[:max_reads * B], log2n, group, rows, r['level'], sm.hann(1 << log2n))


@pytest.mark.parametrize('log2n,group', [(12, 4), (12, 1), (13, 3), (14, 2)])
def test_one_read_per_run(engine_lib, log2n, group):
    m = gated_model(log2n, group)
    r = hm.gated_reference(log2n, group)
    with chan() as ch:
        ch.survey_start(log2n, 'hann')
        before = ch.stat('device_bytes')
        assert ch.stat('survey_groups') == 0
        ch.survey_hold_start(group, 5, r['level'])
        n = 1 << log2n
        assert ch.stat('device_bytes') >= before + n * (8 * 3 + 4 + 8 + 8 * 5)  # gsum, peak, low, busy, level, ring
        one_read_per_run(ch, hm.gated())
        all_equal(ch, m, 'log2n %d group %d' % (log2n, group))
        assert m.hold.gidx == (7 * B >> log2n) // group > 5
        assert ch.stat('survey_groups') == m.hold.gidx
        assert ch.stat('survey_launches') == 3 * 7
        hold_equal(ch.survey_hold_read(), (r['peak'], r['low'], r['busy'], r['groups']), 'the cached reference')
        ch.survey_hold_stop()
        assert ch.stat('device_bytes') == before


def test_group_longer_than_a_run(engine_lib):
    """40 segments per group, 14 per run: a group spans three runs, two groups in 98 segments"""
    x = hm.gated()
    m = hm.run_model(x, 12, 40, 3, None, sm.hann(4096))
    assert m.hold.gidx == 2 and m.hold.fill == 18
    with chan() as ch:
        ch.survey_start(12, 'hann')
        ch.survey_hold_start(40, 3)
        one_read_per_run(ch, x[:2 * B])
        got = ch.survey_hold_read()  # 28 segments: no group yet
        assert got[3] == 0 and not got[0].view(np.uint64).any() and np.all(got[1] == np.inf) and not got[2].any()
        rows, first = ch.survey_hold_rows()
        assert rows.shape == (0, 4096) and first == 0
        one_read_per_run(ch, x[2 * B:])
        all_equal(ch, m, 'group 40')
        assert not m.hold.busy.any()  # no level


def test_batches_of_three_reads(engine_lib):
    """max_blocks 3, all 7 reads pushed before one run: batches of 3, 3 and 1"""
    m = gated_model(12, 4)
    with chan(max_blocks=3, host_out=True) as ch:
        ch.survey_start(12, 'hann')
        ch.survey_hold_start(4, 5, hm.gated_reference(12, 4)['level'])
        for r in reads(hm.gated()):
            ch.push(r)
        ch.run()
        all_equal(ch, m, 'batches')
        assert ch.stat('survey_launches') == 3 * 3


def test_hold_started_after_two_reads(engine_lib):
    """group 0 begins with the first segment completed after the call (it holds read 1's tail),
    also when read 1 is pushed and not yet run at the call; the survey's sums are those of a
    survey without a hold"""
    x = hm.gated()
    level = hm.gated_reference(12, 4)['level']
    m = hm.SurveyHoldModel(12, sm.hann(4096))
    m.feed(x[:B])
    m.feed(x[B:2 * B])
    m.hold_start(4, 5, level)
    for r in reads(x[2 * B:]):
        m.feed(r)
    assert m.hold.gidx == (98 - 28) // 4
    with chan(max_blocks=2) as ch:
        ch.survey_start(12, 'hann')
        ch.push(x[:B])
        ch.run()
        ch.push(x[B:2 * B])
        ch.survey_hold_start(4, 5, level)  # runs read 1 without the hold
        assert ch.stat('survey_launches') == 2 * 2
        one_read_per_run(ch, x[2 * B:])
        all_equal(ch, m, 'late start')
        survey_equal(ch.survey_read(), (hm.gated_reference(12, 4)['acc'], 98), 'against no hold')


def test_reset_in_mid_stream(engine_lib):
    x = hm.gated()
    level = hm.gated_reference(13, 3)['level']
    m = hm.SurveyHoldModel(13, sm.hann(8192))
    m.hold_start(3, 5, level)
    with chan() as ch:
        ch.survey_start(13, 'hann')
        ch.survey_hold_start(3, 5, level)
        one_read_per_run(ch, x[:3 * B])
        for r in reads(x[:3 * B]):
            m.feed(r)
        assert m.hold.fill == 0 and m.hold.gidx == 7  # 21 segments
        m.feed(x[3 * B:4 * B])
        one_read_per_run(ch, x[3 * B:4 * B])
        assert m.hold.fill == 1  # 28 segments: a group is unfinished at the reset
        hold_equal(ch.survey_hold_read(reset=True), m.hold.read(reset=True), 'first half')
        got = ch.survey_hold_read()
        assert got[3] == 0 and not got[0].view(np.uint64).any() and np.all(got[1] == np.inf) and not got[2].any()
        rows_equal(ch.survey_hold_rows(), m.hold.read_rows()[:2], 'the ring after the reset')
        survey_equal(ch.survey_read(reset=True), m.read(reset=True), 'the survey')  # does not touch the hold
        hold_equal(ch.survey_hold_read(), m.hold.read(), 'after the survey reset')
        one_read_per_run(ch, x[4 * B:])
        for r in reads(x[4 * B:]):
            m.feed(r)
        all_equal(ch, m, 'second half')  # the unfinished group went on, first_group counts from the start
        assert ch.survey_hold_rows()[1] == m.hold.gidx - 5 == 11
        assert ch.stat('survey_groups') == 16


def test_rows(engine_lib):
    x = hm.gated()
    with chan() as ch:
        ch.survey_start(12, 'hann')
        ch.survey_hold_start(4, 64)  # more rows than groups
        one_read_per_run(ch, x)
        m = gated_model(12, 4, 64)
        rows, first = ch.survey_hold_rows()
        assert rows.shape == (24, 4096) and first == 0 and not ch.hold_rows_full
        same_bits(rows, m.hold.read_rows()[0], 'rows 64')
        rows_equal(ch.survey_hold_rows(cap_rows=24), m.hold.read_rows(24)[:2], 'cap 24')
        assert not ch.hold_rows_full
        rows_equal(ch.survey_hold_rows(cap_rows=7), m.hold.read_rows(7)[:2], 'cap 7')  # the newest 7
        assert ch.hold_rows_full and ch.survey_hold_rows(cap_rows=7)[1] == 17
        rows, first = ch.survey_hold_rows(cap_rows=0)
        assert rows.shape[0] == 0 and first == 24 and ch.hold_rows_full
        ch.survey_hold_stop()
        # a ring that went round: 14 groups in 5 rows, rows 9 .. 13 lie at 4, 0, 1, 2, 3
        ch.survey_hold_start(4, 5)
        one_read_per_run(ch, x[:4 * B])
        m = hm.SurveyHoldModel(12, sm.hann(4096))
        m.feed(x)  # the survey's grid went on: its tail is the whole stream's
        m.hold_start(4, 5)
        for r in reads(x[:4 * B]):
            m.feed(r)
        assert m.hold.gidx == 14
        rows_equal(ch.survey_hold_rows(), m.hold.read_rows()[:2], 'ring')  # around the ring's end
        assert ch.survey_hold_rows()[1] == 9
        rows_equal(ch.survey_hold_rows(cap_rows=2), m.hold.read_rows(2)[:2], 'ring, cap 2')
        assert ch.hold_rows_full and ch.survey_hold_rows(cap_rows=2)[1] == 12
        rows_equal(ch.survey_hold_rows(cap_rows=4), m.hold.read_rows(4)[:2], 'ring, cap 4')


def test_levels(engine_lib):
    """no level: busy stays 0; a level with NaN, infinite and zero entries: the first never exceeded"""
    x = hm.gated()[:4 * B]
    level = np.array(hm.gated_reference(12, 4)['level'])
    level[0::5] = np.nan
    level[1::5] = np.inf
    level[2::5] = 0.0
    level[3::5] = -np.inf
    for lv in (None, level):
        m = hm.run_model(x, 12, 4, 0, lv, sm.hann(4096))
        with chan() as ch:
            ch.survey_start(12, 'hann')
            ch.survey_hold_start(4, 0, lv)
            one_read_per_run(ch, x)
            all_equal(ch, m, 'level %s' % (lv is not None))
            busy = ch.survey_hold_read()[2]
        if lv is None:
            assert not busy.any()
        else:
            assert not busy[0::5].any() and not busy[1::5].any() and not busy[3::5].any()
            assert np.all(busy[2::5] == 14) and 0 < np.count_nonzero(busy[4::5]) < 20


@pytest.mark.parametrize('kind', ['zeros', 'fullscale'])
def test_input_classes(engine_lib, kind):
    x = sm.stream(kind)[:3 * B]
    level = np.zeros(4096)
    m = hm.run_model(x, 12, 4, 2, level)
    with chan() as ch:
        ch.survey_start(12)
        ch.survey_hold_start(4, 2, level)
        one_read_per_run(ch, x)
        all_equal(ch, m, kind)
        peak, low, busy, groups = ch.survey_hold_read()
    assert groups == 10
    if kind == 'zeros':  # exactly +0: 0 < +infinity, and 0 is above no 0
        assert not peak.view(np.uint64).any() and not low.view(np.uint64).any() and not busy.any()
    else:
        assert np.count_nonzero(busy == 10) > 2048 and np.all(peak >= low)


def test_dc_removal(engine_lib):
    """correct_dc_bias: the hold sees the survey's stream, after dc_kernel"""
    x = sm.stream('dc', nreads=3)
    m = hm.run_model(sm.dc_remove(x), 12, 4, 3)
    with chan(max_blocks=2, dcc=True) as ch:
        ch.survey_start(12)
        ch.survey_hold_start(4, 3)
        ch.push(x[:2 * B])
        ch.run()
        ch.push(x[2 * B:])
        ch.run()
        all_equal(ch, m, 'dc')


def test_second_read_length(engine_lib):
    """1.536 Msps: reads of 384000 samples, 23.4 segments of 16384 each, groups of 5"""
    cfg = tl.PUB_CONFIGS['r1536k']
    x = sm.stream('tones', 1536000, 2, 384000)
    m = hm.run_model(x, 14, 5, 4, None, None, 384000)
    assert m.hold.gidx == 9
    with chan(cfg=cfg) as ch:
        assert ch.block_len == 384000
        ch.survey_start(14)
        ch.survey_hold_start(5, 4)
        one_read_per_run(ch, x, 384000)
        all_equal(ch, m, 'r1536k')


def test_lifecycle_and_errors(engine_lib):
    import aero_engine as ae
    x = hm.gated()

    def refused(f, *a):
        with pytest.raises(ae.AeroError) as e:
            f(*a)
        assert e.value.rc == ae.AERO_E_INVALID

    with chan() as ch:
        base = ch.stat('device_bytes')
        refused(ch.survey_hold_start, 4)  # no survey
        refused(ch.survey_hold_read)
        refused(ch.survey_hold_rows)
        refused(ch.survey_hold_stop)
        ch.survey_start(12, 'hann')
        with_survey = ch.stat('device_bytes')
        refused(ch.survey_hold_read)  # a survey and no hold
        refused(ch.survey_hold_rows)
        refused(ch.survey_hold_stop)
        for group, rows in ((0, 0), (65537, 0), (-1, 0), (4, -1), (4, 4097)):
            refused(ch.survey_hold_start, group, rows)
            assert ch.stat('device_bytes') == with_survey
        one_read_per_run(ch, x[:B])
        assert ch.stat('survey_launches') == 2 and ch.stat('survey_groups') == 0
        ch.survey_hold_start(65536, 4096)  # the largest of both
        ch.survey_hold_stop()
        ch.survey_hold_start(4)
        refused(ch.survey_hold_start, 4)  # a second one
        refused(ch.survey_hold_rows)  # rows == 0
        assert ch.stat('device_bytes') > with_survey
        one_read_per_run(ch, x[B:3 * B])
        assert ch.stat('survey_launches') == 2 + 3 * 2
        assert ch.stat('survey_groups') == ch.survey_hold_read()[3] == 7  # segments 14 .. 41 of the survey
        ch.survey_hold_stop()
        assert ch.stat('device_bytes') == with_survey
        refused(ch.survey_hold_read)
        one_read_per_run(ch, x[3 * B:5 * B])  # the survey goes on unchanged
        assert ch.stat('survey_launches') == 2 + 3 * 2 + 2 * 2 and ch.stat('survey_groups') == 7
        m = sm.SurveyModel(12, sm.hann(4096))
        m.feed(x[:5 * B])
        survey_equal(ch.survey_read(), m.read(), 'after hold_stop')
        ch.survey_hold_start(2, 3, np.zeros(4096))  # a fresh one: its own grid and index
        one_read_per_run(ch, x[5 * B:6 * B])
        assert ch.survey_hold_rows()[1] == 7 - 3 and ch.stat('survey_groups') == 7 + 7
        ch.survey_stop()  # ends the hold
        assert ch.stat('device_bytes') == base
        refused(ch.survey_hold_read)
        refused(ch.survey_hold_stop)
        ch.survey_start(13)
        refused(ch.survey_hold_read)
        ch.survey_hold_start(1)
        one_read_per_run(ch, x[6 * B:])
        assert ch.survey_hold_read()[3] == 7
        import ctypes
        peak, low, groups = np.zeros(8192), np.zeros(8192), ctypes.c_uint64()
        rc = ch.lib.aero_chan_survey_hold_read(ch.h, peak.ctypes.data, low.ctypes.data, None, 8191, ctypes.byref(groups), 0)
        assert rc == ae.AERO_E_INVALID  # cap below N
        rc = ch.lib.aero_chan_survey_hold_read(ch.h, peak.ctypes.data, low.ctypes.data, None, 8192, ctypes.byref(groups), 0)
        assert rc == ae.AERO_OK and groups.value == 7 and np.all(peak >= low)  # busy may be NULL


def _audio_equal(ch, ref, cfg, what):
    for v in range(len(cfg['vfos'])):
        want, got = ref.usb(v), ch.audio(v)
        assert len(want) > 0 and np.array_equal(want, got), '%s: audio of vfo %d' % (what, v)
    for m in range(len(cfg['mains'])):
        assert np.array_equal(ref.iq(m), ch.iq(m)), '%s: IQ of main %d' % (what, m)


def test_audio_does_not_change(engine_lib):
    """a hold that starts and stops in mid-stream: every VFO's audio is the oracle publisher's"""
    x = sm.stream('tones', nreads=5)
    ref = tl.OraclePublisher(FS, C, CFG['mains'], CFG['vfos'], correct_dc_bias=False)
    ref.process(x)
    m = hm.SurveyHoldModel(12, sm.hann(4096))
    with chan(max_blocks=2, host_out=True) as ch:
        for b, r in enumerate(reads(x)):
            if b == 1:
                ch.survey_start(12, 'hann')  # runs read 0 without it
            if b == 2:
                ch.survey_hold_start(4, 2, np.zeros(4096))  # runs read 1 without it
                m.feed(x[B:2 * B])
                m.hold_start(4, 2, np.zeros(4096))
            if b == 4:
                ch.run()
                m.feed(x[2 * B:3 * B])
                m.feed(x[3 * B:4 * B])
                all_equal(ch, m, 'reads 2 and 3')
                ch.survey_hold_stop()
            ch.push(r)
        ch.run()
        ch.sync()
        assert ch.stat('survey_groups') == m.hold.gidx > 0
        _audio_equal(ch, ref, CFG, 'hold on')
