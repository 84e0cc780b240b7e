"""What the streams of tests/burst_inputs.py reach in the burst demodulators
and the R/T framing, shown with the oracle alone, fed one 16384-sample message
at a time as tests/test_gpu_burst_inputs.py's first schedule pushes them: more
trident checks in one message than the front end has slots (TRI_SLOTS), more
R/T tests in one message than a framing lane queues per pass
(RT_TESTS_PER_PASS), an R/T block filled to its last test (blockptr
RT_BLOCK), accepted checks with and without a start-of-packet marker, checks
that are all rejected, a UW and R/T tests without a packet, a burst behind an
AGC ring of zeros, DataCarrierDetect dropped by the 1-s timer alone; and the
plain synthetic stream reaches none of the bounded resources.  These are
conditions on the inputs: if one fails, the class is changed, not the
condition."""
import numpy as np
import pytest

import burst_inputs as bi

KINDS = list(bi.KINDS)
MSK = [k for k in KINDS if k.startswith('msk')]


@pytest.fixture(scope='module')
def reach(cpu_libs):
    """(kind, class, tick) -> bi.facts of the class under the 'max' schedule, computed once"""
    cache = {}

    def get(kind, name, tick=False):
        if (kind, name, tick) not in cache:
            cache[kind, name, tick] = bi.facts(kind, dict(bi.streams(kind))[name], 'max', tick)
        return cache[kind, name, tick]
    return get


@pytest.mark.parametrize('kind', KINDS)
def test_class_list_and_lengths(kind, cpu_libs):
    got = dict(bi.streams(kind))
    names = [n for n, _ in bi.streams(kind)]
    assert tuple(names) == bi.ORDER
    i = names.index('pulse_stall')  # unlike neighbours: silence | the stalling pulse train | full scale | 1 LSB
    assert names[i - 1] == 'silence' and names[i + 1:i + 3] == ['square', 'lsb_noise']
    for name, x in got.items():
        assert x.dtype == np.int16 and not x.flags.writeable
        if name not in ('late', 'cut_silence'):
            assert len(x) == bi.LEN == 3 * bi.FS + bi.TAIL, name
    assert len(got['late']) % bi.MAX_MSG == (bi.LATE_LEAD + bi.TAIL) % bi.MAX_MSG
    assert len(got['late']) <= bi.LATE_LEAD + bi.LEN
    assert len(got['cut_silence']) % bi.FS == bi.TAIL and bi.LEN <= len(got['cut_silence']) <= 8 * bi.FS + bi.TAIL
    assert not got['silence'].any() and np.count_nonzero(got['one_sample']) == 1
    assert set(np.unique(got['lsb_noise'])) == {-1, 0, 1}
    assert set(np.unique(got['square'])) == {-32768, 32767} and set(np.unique(got['const_min'])) == {-32768}
    assert (got['square'][:12] == [32767] * 3 + [-32768] * 3 + [32767] * 3 + [-32768] * 3).all()  # period 6
    assert got['clip'].max() == 32767 and got['clip'].min() == -32768
    assert np.abs(got['tiny'].astype(int)).max() <= 32768 // 2048
    syn = got['synth'].astype(int)
    assert (got['negated'] == np.clip(-syn, -32768, 32767)).all()
    assert not got['late'][:bi.LATE_LEAD].any() and got['late'][bi.LATE_LEAD:].any()
    for fill, v in (('silence', 0), ('fullscale', 32767)):
        x, cut = bi.cut_stream(kind, fill)
        assert (x[:cut] == got['synth'][:cut]).all() and (x[cut:] == v).all()


def test_schedules():
    for n in (bi.LEN, bi.LATE_LEAD + bi.MAX_MSG + bi.TAIL):
        for schedule in bi.SCHEDULES:
            flat = [m for grp in bi.runs(n, schedule) for m in grp]
            assert flat[0][0] == 0 and flat[-1][1] == n and all(a[1] == b[0] for a, b in zip(flat, flat[1:]))
            assert all(0 < b - a <= bi.MAX_MSG for a, b in flat)
        assert all(len(g) == 1 for g in bi.runs(n, 'max')) and bi.runs(n, 'max')[0] == [(0, 16384)]
        assert [b - a for a, b in bi.runs(n, 'queued')[0]] == [16383, 16383]
        sizes = [b - a for grp in bi.runs(n, 'ragged') for a, b in grp]
        assert sizes[:8] == [6144, 6145, 6146, 1, 12000, 2047, 16384, 37] and sizes.count(1) >= 2


def test_pulse_stall_reaches_every_bound(reach):
    f = reach('oqpsk10500', 'pulse_stall')
    assert f['checks_msg'] > bi.TRI_SLOTS, 'more trident checks in one message than the front end has slots'
    assert f['tests_msg'] > bi.RT_TESTS_PER_PASS, 'more R/T tests in one message than a lane queues per pass'
    assert f['blockptr'] == bi.RT_BLOCK == 320 + 192 * 30, 'an R/T block filled to its last test'
    assert 0 < f['marks'] < f['accepted'], 'accepted checks with and without a start-of-packet marker'
    assert f['soft'] > 16384, 'more soft bits than the soft ring holds'
    assert 1400 <= bi.stall_stream('oqpsk10500')[1] <= 1600


@pytest.mark.parametrize('kind', KINDS)
def test_plain_synth_reaches_none_of_them(kind, reach):
    """the gap: what every GPU test of the burst path fed until now"""
    f = reach(kind, 'synth')
    assert f['packets'] >= 1 and f['accepted'] >= 1, 'it decodes'
    assert f['checks_msg'] < bi.TRI_SLOTS and f['tests_msg'] < bi.RT_TESTS_PER_PASS and f['blockptr'] < bi.RT_BLOCK
    assert f['marks'] == f['accepted'] and f['soft'] < 16384


@pytest.mark.parametrize('kind', MSK)
def test_msk_pulse_train(kind, reach):
    """burst MSK checks lie too far apart to fill the slots: the class with the most in one message, all rejected"""
    f = reach(kind, 'pulse_stall')
    assert f['checks'] > 3 * reach(kind, 'synth')['checks'] and f['checks_msg'] >= 2
    assert f['checks_msg'] <= bi.TRI_SLOTS and not f['accepted'] and not f['soft']
    assert 5000 <= bi.stall_stream(kind)[1] <= 6000


@pytest.mark.parametrize('kind', KINDS)
def test_rejected_pulse_trains(kind, reach):
    f = reach(kind, 'pulse_reject')
    assert f['checks'] >= 9 and not f['accepted'] and not f['soft'] and not f['tests']
    assert bi.reject_stream(kind)[1] != bi.stall_stream(kind)[1]
    g = reach(kind, 'noise_pulse')
    if kind == 'oqpsk10500':  # a retrigger while a buffer fills, one check accepted on noise, tests on its soft bits
        assert g['checks_msg'] > bi.TRI_SLOTS and 1 <= g['accepted'] < g['checks'] and g['tests'] >= 1
        assert not g['packets']
    else:
        assert g['checks'] > reach(kind, 'noise')['checks'] and not g['accepted']


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('fill', ['silence', 'fullscale', 'noise'])
def test_cut_bursts(kind, fill, reach):
    """the UW found, R/T tests run, the packet lost"""
    f, whole = reach(kind, 'cut_' + fill), reach(kind, 'synth')
    assert f['edges'] >= 1 and f['accepted'] >= 1 and f['tests'] >= 1 and f['packets'] < whole['packets']
    cut = bi.cut_stream(kind, fill)[1]
    back = bi.CUT_SEARCH[bi.KINDS[kind][0]][0]
    assert bi.first_accept(kind) - back <= cut < bi.first_accept(kind)  # inside the burst the check belongs to
    if kind == 'oqpsk10500' and fill == 'fullscale':  # the second class that runs a block to its end
        assert f['blockptr'] == bi.RT_BLOCK and f['tests_msg'] > bi.RT_TESTS_PER_PASS


@pytest.mark.parametrize('kind', KINDS)
def test_overlapping_bursts(kind, reach):
    f, whole = reach(kind, 'overlap'), reach(kind, 'synth')
    assert f['accepted'] >= 1 and f['tests'] >= 1
    if kind == 'oqpsk10500':
        assert f['checks'] > whole['checks'] and f['accepted'] > whole['accepted']
        assert f['tests_msg'] > bi.RT_TESTS_PER_PASS and f['checks_msg'] == bi.TRI_SLOTS  # every slot, no stall
    else:  # the second burst spoils the first: tests, no packet
        assert f['packets'] == 0 < whole['packets']


@pytest.mark.parametrize('kind', KINDS)
def test_scaled_and_shifted_bursts(kind, reach):
    whole = reach(kind, 'synth')
    for name in ('clip', 'tiny', 'negated'):
        f = reach(kind, name)
        assert f['accepted'] >= 1 and f['soft'] > 0 and f['tests'] >= 1, name
    if kind == 'oqpsk10500':
        assert reach(kind, 'clip')['tests'] > whole['tests'] and reach(kind, 'tiny')['soft'] != whole['soft']
        assert reach(kind, 'lead0')['accepted'] >= 1 and reach(kind, 'lead0')['checks_msg'] > whole['checks_msg']
        assert reach(kind, 'late')['packets'] >= 1, 'the burst behind an AGC ring of zeros decodes'
    else:  # a burst from sample 0 and one behind an AGC ring of zeros: checked and rejected
        for name in ('lead0', 'late'):
            f = reach(kind, name)
            assert f['checks'] >= 2 and not f['accepted'] and not f['soft'], name


@pytest.mark.parametrize('kind', KINDS)
def test_silent_classes_give_no_soft_bits(kind, reach):
    for name in bi.SILENT:
        f = reach(kind, name)
        assert 1 <= f['checks'] <= 4 and not f['accepted'], name
        assert not f['soft'] and not f['marks'] and not f['tests'] and not f['edges'], name
    f = reach(kind, 'noise')
    assert f['checks'] >= 2 and not f['accepted'] and not f['soft']


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('tick', [False, True])
def test_every_record_is_finite(kind, tick, reach):
    for name in bi.ORDER:
        assert reach(kind, name, tick)['finite'], name


@pytest.mark.parametrize('kind', KINDS)
def test_dcd_timer_shows(kind, reach):
    """the tick leg is not vacuous: on cut_silence only the timer drops DataCarrierDetect"""
    changed = [n for n in bi.ORDER if reach(kind, n, True)['edges'] != reach(kind, n)['edges']]
    assert 'cut_silence' in changed
    assert reach(kind, 'cut_silence', True)['edges'] == reach(kind, 'cut_silence')['edges'] + 1


def test_message_cuts_show(cpu_libs):
    """burst output depends on the message boundaries: the schedules are different references"""
    x = dict(bi.streams('oqpsk10500'))['pulse_stall']
    a, b = bi.walk('oqpsk10500', x, 'max')[0], bi.walk('oqpsk10500', x, 'ragged')[0]
    assert len(a['soft']) != len(b['soft']) or not np.array_equal(a['soft'], b['soft'])
