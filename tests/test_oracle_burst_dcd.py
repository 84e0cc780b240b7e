"""The model AERO_F_DCD_TICK_BURST is checked against: the oracle with AeroL's
1 s DCD timer slot run between messages (tests/oracle_tick.py).

In burst mode a sync sets datacd and a countdown of 12; the burst window ends
only after 10500 soft bits, several bursts later, and until then the UW search
is gated by datacd.  The timer takes the countdown 12 -> 9 -> 6 -> 3 -> 0 and
clears datacd at the fourth tick after a sync, which reopens the search for the
next burst: the ticked model decodes packets the untimed one misses.  The
counts below were measured with this oracle and hook on the three 60-s streams
at 12000-sample messages; the demodulator never reads datacd, so the delivered
soft bits are the same with and without the timer.  Burst MSK does not gate
its sync on datacd: there the timer only adds DataCarrierDetect changes."""
import numpy as np
import pytest

import aero_testlib as tl
import oracle_tick as ot

# (seconds, seed, Eb/N0 dB): untimed (packets, items), ticked (packets, items)
STREAMS = {(60, 2, 14.0): ((12, 8), (13, 9)),
           (60, 0xAE50, 12.0): ((11, 7), (14, 9)),
           (60, 7, 10.0): ((12, 8), (14, 9))}


@pytest.fixture(scope='module')
def runs(cpu_libs):
    out = {}
    for (sec, seed, db) in STREAMS:
        pcm, pk = tl.synth_burst(seconds=float(sec), seed=seed, carrier=12000.0, ebn0=db, return_packets=True)
        out[(sec, seed, db)] = dict(sent=pk, untimed=ot.run(pcm, 12000, tick=False), ticked=ot.run(pcm, 12000))
    return out


@pytest.fixture(scope='module')
def msk_runs(cpu_libs):
    pcm = tl.synth_burst_msk(seconds=20.0, bitrate=1200, seed=0xAE70)
    return {size: (ot.run(pcm, size, bitrate=1200, tick=False), ot.run(pcm, size, bitrate=1200))
            for size in (12000, 4800, 7000)}


def test_hooked_library_without_ticks_is_the_oracle(cpu_libs):
    pcm = tl.synth_burst(seconds=12.0, seed=7, carrier=12000.0, ebn0=10.0)
    ref = tl.Oracle(burst=True)
    ref.push_chunked(pcm, 12000)
    got = ot.run(pcm, 12000, tick=False)
    assert len(got['soft']) > 1000 and np.array_equal(got['soft'], ref.softbits16())
    assert len(got['tests']) and np.array_equal(got['tests'], ref.rt_tests())
    assert got['packets'] and got['packets'] == ref.rt_packets()
    assert got['items'] == ref.item_lines('A')
    assert got['edges'] == ref.events()[0]


@pytest.mark.parametrize('key', sorted(STREAMS), ids=lambda k: '%ds-seed%x-%gdB' % k)
def test_timer_reopens_the_uw_search(runs, key):
    (up, ui), (tp, ti) = STREAMS[key]
    u, t = runs[key]['untimed'], runs[key]['ticked']
    assert (len(u['packets']), len(u['items'])) == (up, ui)
    assert (len(t['packets']), len(t['items'])) == (tp, ti)
    assert np.array_equal(u['soft'], t['soft']), 'the demodulator read datacd'
    assert u['edges'] == 1 and t['edges'] > 1


@pytest.mark.parametrize('key', sorted(STREAMS), ids=lambda k: '%ds-seed%x-%gdB' % k)
def test_ticked_packets_were_transmitted(runs, key):
    pk = runs[key]['sent']
    for kind, info in runs[key]['ticked']['packets']:
        if kind == 'R':  # 20 bytes: the 19 sent + the tail byte
            assert any(k == 'R' and info[:19] == b for k, b in pk)
        else:  # T: chop(1) drops the tail byte
            assert any(k == 'T' and info[:len(b)] == b for k, b in pk)


@pytest.mark.parametrize('size', [12000, 4800, 7000])
def test_burst_msk_timer_only_adds_dcd_edges(msk_runs, size):
    u, t = msk_runs[size]
    assert (u['edges'], t['edges']) == (1, 4)
    assert len(u['tests']) and np.array_equal(u['tests'], t['tests'])
    assert u['packets'] and u['packets'] == t['packets']
    assert u['items'] == t['items']
    assert np.array_equal(u['soft'], t['soft'])
