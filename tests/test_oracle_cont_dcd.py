"""The model AERO_F_DCD_TICK_CONT is checked against (tests/cont_dcd_lib.py),
pinned on the CPU before any GPU runs:

* the outage streams give the DataCarrierDetect edge counts measured with the
  oracle: 1 without the timer whatever happens to the carrier, more with it;
* soft bits, hops, frames, items (C: Call_progress SUs, voice) do not depend on
  the timer: neither framing reads datacd;
* the MSK model (the hooked oracle fed the stream cut at the tick samples) is
  chunk-invariant, also across rate changes in the middle of a timer second;
* for the C channel, the hook at the ends of messages that divide 48000 and
  the oracle's own sample-clock timer agree;
* the host's countdown walk over one pass (dcd_host.h through
  tools/hostcheck.cpp): hand-made orders of tick, sync and frame end.
"""
import ctypes
import os

import numpy as np
import pytest

import aero_testlib as tl
import cont_dcd_lib as cd

pytestmark = pytest.mark.usefixtures('cpu_libs')


def _same_but_edges(a, b, keys):
    for k in keys:
        if isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


MSK_KEYS = ('soft', 'hops', 'frames', 'items')
C_KEYS = ('soft', 'pt', 'hops', 'frames', 'c_units', 'voice')


@pytest.mark.parametrize('name', sorted(cd.MSK_ROWS))
def test_msk_outage_edges(name):
    r = cd.MSK_ROWS[name]
    pcm, fs = cd.msk_stream(name), r['fs']
    plain, _ = cd.msk_run([(pcm, fs)], r['bitrate'], fs, fs // 10, tick=False)
    ticked, o = cd.msk_run([(pcm, fs)], r['bitrate'], fs, fs // 10, tick=True)
    assert o.ticks == len(pcm) // fs
    assert len(plain['soft']) > 5000 and len(plain['frames']) > 0, 'the oracle did not lock'
    assert plain['edges'] == r['untimed'] == 1
    assert ticked['edges'] == r['ticked'] and r['ticked'] > 1
    _same_but_edges(plain, ticked, MSK_KEYS)


def test_msk_carrier_then_noise():
    a = tl.synth_msk(seconds=20.0, bitrate=600, seed=0xAE40)
    pcm = np.concatenate([a, cd.noise_like(a, 10.0, 12000, 0xAE40)])
    plain, _ = cd.msk_run([(pcm, 12000)], 600, 12000, 1200, tick=False)
    ticked, _ = cd.msk_run([(pcm, 12000)], 600, 12000, 1200, tick=True)
    assert (plain['edges'], ticked['edges']) == (1, 2)  # with the timer the carrier is lost, for good
    _same_but_edges(plain, ticked, MSK_KEYS)


def test_rescale_rule():
    assert cd.rescale(12000, 12000, 16000) == 16000  # nothing elapsed
    assert cd.rescale(1, 12000, 16000) == 16000 - (11999 * 16000) // 12000 == 2
    assert cd.rescale(7200, 12000, 16000) == 16000 - 6400
    clk = cd.TickClock(12000)
    assert clk.cuts(30000) == [12000, 24000] and clk.left == 6000
    clk.set_rate(16000)
    assert clk.left == 8000 and clk.cuts(8000) == [8000] and clk.left == 16000


@pytest.mark.parametrize('name', ['12000-16000-12000', '24000-40000'])
def test_msk_rate_change_chunk_invariant(name):
    bitrate, segs = cd.rate_change_segments(name)
    fs0 = segs[0][1]
    plain, _ = cd.msk_run(segs, bitrate, fs0, None, tick=False)
    ref, o = cd.msk_run(segs, bitrate, fs0, None, tick=True)
    assert o.ticks == cd.model_ticks(segs, fs0)
    # the rate changes fall inside a timer second: the rescale rule is in play
    clk = cd.TickClock(fs0)
    for pcm, fs in segs[:-1]:
        clk.set_rate(fs)
        clk.cuts(len(pcm))
        assert clk.left != fs
    assert len(ref['soft']) > 5000 and len(ref['frames']) > 0
    assert ref['edges'] != plain['edges'] == 1
    _same_but_edges(plain, ref, MSK_KEYS)
    for size in (1000, 3333):
        got, o2 = cd.msk_run(segs, bitrate, fs0, size, tick=True)
        assert o2.ticks == o.ticks
        assert got['edges'] == ref['edges'], size
        _same_but_edges(ref, got, MSK_KEYS)


@pytest.mark.parametrize('name', ['12000-16000-12000', '24000-40000'])
def test_msk_rate_change_streams_tell_the_rule(name):
    """A copy truncated at the model's tick sample of a fall after the rate
    change has one edge more than under a second that restarts at the rate
    change, and than a copy one sample shorter (what the GPU test decodes)."""
    bitrate, segs = cd.rate_change_segments(name)
    fs0 = segs[0][1]
    stop, edges = cd.rule_witness(segs, bitrate, fs0)
    assert len(segs[0][0]) < stop < sum(len(p) for p, _ in segs)
    got = [cd.msk_run(segs, bitrate, fs0, None, stop=s, rule=r)[0]['edges']
           for s, r in ((stop, 'rescale'), (stop, 'restart'), (stop - 1, 'rescale'))]
    assert got == [edges, edges - 1, edges - 1]


def test_c_outage_edges():
    pcm, quiet_end = cd.c_outage()
    msgs = tl.cut(pcm, (4800,))
    plain = cd.c_run(msgs, tick=False)
    ticked = cd.c_run(msgs, tick=True)
    assert tl.c_produced(plain)
    assert (plain['edges'], ticked['edges']) == (1, 3)
    _same_but_edges(plain, ticked, C_KEYS)
    # the hook at the ends of the messages that complete a second: the same model
    hooked = cd.c_run(msgs, tick=True, hooked=True)
    assert hooked['edges'] == ticked['edges']
    _same_but_edges(ticked, hooked, C_KEYS)
    # the call's end is visible: an even edge count once the quiet part is over
    assert cd.c_run(tl.cut(pcm[:quiet_end], (4800,)), tick=True)['edges'] == 2


@pytest.mark.parametrize('ebn0', [12.0, 6.0])
def test_c_steady_carrier_keeps_dcd(ebn0):
    pcm = tl.synth_c(seconds=14.0, seed=0xC1A5, carrier=11000.0, ebn0=ebn0)
    msgs = tl.cut(pcm, (4800,))
    assert cd.c_run(msgs, tick=False)['edges'] == 1
    assert cd.c_run(msgs, tick=True)['edges'] == 1


# ---------------------------------------------------------------- the host's walk
@pytest.fixture(scope='module')
def dcd_pass():
    so = os.environ.get('AERO_HOSTCHECK_SO')
    if not so:
        import build
        so = build.build_hostcheck()
    L = ctypes.CDLL(so)
    L.hc_dcd_pass.argtypes = [ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                              ctypes.c_int, ctypes.c_int]
    L.hc_dcd_pass.restype = None

    def run(state, syncs=(), jobs=(), down=3, tick=False):
        """state (countdown, datacd, edges); syncs: jobs listed before each sync;
        jobs: None (a block that ends no frame) or the frame's SU CRC results"""
        st = np.array(state, dtype=np.int32)
        word = len(syncs)
        for k, before in enumerate(syncs):
            word |= before << (4 + 2 * k)
        nsu = np.array([-1 if j is None else len(j) for j in jobs] + [0], dtype=np.int32)
        masks = np.array([0 if j is None else sum(1 << k for k, ok in enumerate(j) if ok) for j in jobs] + [0],
                         dtype=np.uint32)
        L.hc_dcd_pass(st.ctypes.data, word, nsu.ctypes.data, masks.ctypes.data, len(jobs), down, int(tick))
        return tuple(int(v) for v in st)
    return run


def test_host_tick_after_frame_end(dcd_pass):
    # two failed SUs take 3 to 0, the pass's tick then drops datacd
    assert dcd_pass((3, 1, 1), jobs=[[False, False]], tick=True) == (0, 0, 2)
    # two good SUs first: 3 -> 7, the tick takes 3 off and datacd stays
    assert dcd_pass((3, 1, 1), jobs=[[True, True]], tick=True) == (4, 1, 1)


def test_host_tick_before_frame_end(dcd_pass):
    # the tick ended the previous pass: datacd falls, and the frame's second good SU raises it again
    s = dcd_pass((3, 1, 1), tick=True)
    assert s == (0, 0, 2)
    assert dcd_pass(s, jobs=[[True, True]]) == (4, 1, 3)


def test_host_countdown_quirk(dcd_pass):
    # updateDCD takes 2 to -1; datacd holds until the next tick clamps it to 0
    s = dcd_pass((2, 1, 1), tick=True)
    assert s == (-1, 1, 1)
    assert dcd_pass(s, jobs=[[True]]) == (1, 1, 1)  # a good SU in between counts from -1
    s = dcd_pass(s, tick=True)
    assert s == (0, 0, 2)
    assert dcd_pass(s, tick=True) == (0, 0, 2)


def test_host_sync_after_fall(dcd_pass):
    fallen = (0, 0, 2)
    assert dcd_pass(fallen, syncs=[0]) == (12, 1, 3)
    # a sync before the pass's frame end, and after it
    assert dcd_pass(fallen, syncs=[0], jobs=[[False]]) == (9, 1, 3)
    assert dcd_pass(fallen, syncs=[1], jobs=[[False]]) == (12, 1, 3)
    # blocks that end no frame count as jobs; the tick comes last
    assert dcd_pass(fallen, syncs=[1], jobs=[None, [False]], tick=True) == (6, 1, 3)
    assert dcd_pass((12, 1, 1), syncs=[0, 1], jobs=[[False, False]]) == (12, 1, 1)
    # the C channel's SUs take 5 off
    assert dcd_pass((12, 1, 1), jobs=[[False, True, False]], down=5, tick=True) == (1, 1, 1)
