"""The persistent coarse kernel (coarse.hip): one workgroup walking through
several channels.

The 16384-point kinds launch at most AERO_COARSE_GRID workgroups (default:
the device's CU count), each taking channels b, b + grid, ... (coarse_sched.h),
so a handful of channels loop once the grid is set below their number.  The
walk must not change a bit: hop records (the ring image, the fold's argmax and
the hop control behind them), soft bits, items and the final smoothed
spectrum y (aero_channel_coarse_y) equal the CPU
oracle's (decode/coarsefreqestimate.cpp:89-150,
decode/oqpskdemodulator.cpp:562-620) whatever the grid is."""
import concurrent.futures as cf

import numpy as np
import pytest

import aero_testlib as tl

pytestmark = pytest.mark.gpu

# carrier Hz, Eb/N0 dB, samples per push.  7020 and 15500 Hz are outside the
# first search window: the hunter steps and the AFC retunes (zero_before,
# yreset, emptyingcountdown).  The push sizes put the channels out of step:
# in one run() some are due and others not, a workgroup's first channel may be
# the one that is not, and a push ending on the hop sample (4096, 4097 vs
# 4095) takes the ring fix-up.
FIVE = [(12037.5, 12.0, 1000), (12038.0, 12.0, 4095), (7020.0, 12.0, 4096), (15500.0, 12.0, 4097),
        (12040.0, 9.0, 30000)]
SECONDS = 8.0


def _oracle(pcm, bitrate=10500):
    o = tl.Oracle(bitrate=bitrate)
    o.push_chunked(pcm, 12000)
    return o.softbits(), o.hops(), (o.c_units() if bitrate == 8400 else o.item_lines('A')), o.coarse_y()


def _oracles(streams, bitrate=10500):
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(lambda s: _oracle(s, bitrate), streams))


@pytest.fixture(scope='module')
def five(cpu_libs):
    streams = [tl.synth(seconds=SECONDS, seed=0xC0A0 + k, carrier=f, ebn0=eb) for k, (f, eb, _) in enumerate(FIVE)]
    return streams, _oracles(streams)


def _run(ae, streams, chunks, flags, bitrate=10500):
    """Pushes every stream in its own chunk size, one run() per round."""
    eng = ae.Engine(max_channels=len(streams), flags=flags)
    chans = [eng.open_channel(bitrate, 48000) for _ in streams]
    pos = [0] * len(streams)
    while any(p < len(s) for p, s in zip(pos, streams)):
        for k, (s, ch) in enumerate(zip(streams, chans)):
            if pos[k] < len(s):
                eng.push(ch, s[pos[k]:pos[k] + chunks[k]])
                pos[k] += chunks[k]
        eng.run()
    eng.flush()
    return eng, chans


def _outputs(eng, chans):
    out = [(eng.softbits(ch), eng.hops(ch), eng.items(ch), eng.channel_coarse_y(ch)) for ch in chans]
    eng.close()
    return out


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.fixture(scope='module')
def five_by_grid(engine_lib, five):
    """The five streams at grid 1 (one workgroup, five iterations), 2 (three
    and two) and 8 (no looping)."""
    import aero_engine as ae
    streams, _ = five
    mp = pytest.MonkeyPatch()
    res = {}
    try:
        for grid in (1, 2, 8):
            mp.setenv('AERO_COARSE_GRID', str(grid))
            res[grid] = _outputs(*_run(ae, streams, [c[2] for c in FIVE], ae.F_TRACE_SOFT | ae.F_TRACE_HOPS))
    finally:
        mp.undo()
    return res


def test_looping_uneven_split_out_of_step(five, five_by_grid):
    _, refs = five
    got = five_by_grid[2]
    for k, ((sb, h, items, (first, y)), (rsb, rh, ritems, ry)) in enumerate(zip(got, refs)):
        assert len(rh) >= int(SECONDS * 48000) // 4096 - 1
        assert _same(h, rh), 'channel %d hop records differ' % k
        assert _same(y, ry[first:first + len(y)]), 'channel %d final y differs' % k
        assert np.array_equal(sb, rsb), 'channel %d soft bits differ' % k
        assert items == ritems, 'channel %d items differ' % k
    assert len(refs[0][0]) > 1000 and refs[0][2], 'oracle did not lock on the plain channel'
    for k in (2, 3):  # the retunes happened: the centre frequency moved
        assert len(np.unique(refs[k][1][:, 3])) > 1, 'channel %d never retuned' % k


def test_grid_independence(five_by_grid):
    for grid in (1, 8):
        for k, (a, b) in enumerate(zip(five_by_grid[grid], five_by_grid[2])):
            assert _same(a[1], b[1]), 'grid %d channel %d hop records differ' % (grid, k)
            assert np.array_equal(a[0], b[0]), 'grid %d channel %d soft bits differ' % (grid, k)
            assert a[2] == b[2]
            assert a[3][0] == b[3][0] and _same(a[3][1], b[3][1]), 'grid %d channel %d final y differs' % (grid, k)


def test_c_channel_loops(engine_lib, monkeypatch):
    import aero_engine as ae
    monkeypatch.setenv('AERO_COARSE_GRID', '2')
    streams = [tl.synth_c(seconds=SECONDS, seed=0xC0B0 + k, carrier=f, ebn0=eb)
               for k, (f, eb) in enumerate(((12037.5, 12.0), (15500.0, 10.0), (9050.0, 8.0)))]
    refs = _oracles(streams, 8400)
    eng, chans = _run(ae, streams, [12000] * 3, ae.F_TRACE_SOFT | ae.F_TRACE_HOPS, bitrate=8400)
    for k, ch in enumerate(chans):
        rsb, rh, rcu, ry = refs[k]
        assert len(rh) > 80 and _same(eng.hops(ch), rh), 'channel %d hop records differ' % k
        first, y = eng.channel_coarse_y(ch)
        assert _same(y, ry[first:first + len(y)]), 'channel %d final y differs' % k
        assert np.array_equal(eng.softbits(ch), rsb), 'channel %d soft bits differ' % k
        assert np.array_equal(eng.c_units(ch), rcu), 'channel %d Call_progress SUs differ' % k
    eng.close()


def test_nothing_due(engine_lib, five, monkeypatch):
    """A push too short to reach a hop boundary: run() returns, no hop is
    recorded, and the full pushes after it give the oracle's hops."""
    import aero_engine as ae
    monkeypatch.setenv('AERO_COARSE_GRID', '2')
    streams, refs = five
    eng = ae.Engine(max_channels=5, flags=ae.F_TRACE_HOPS)
    chans = [eng.open_channel(10500, 48000) for _ in streams]
    pos = 2 * 4096 + 100
    for s, ch in zip(streams, chans):
        eng.push(ch, s[:pos])
    eng.run()
    eng.sync()
    got = [[eng.hops(ch)] for ch in chans]  # hops() pops what was recorded since the last call
    assert [len(g[0]) for g in got] == [2] * 5
    for s, ch in zip(streams, chans):  # 9292 samples so far: the third hop sample is 12287
        eng.push(ch, s[pos:pos + 1000])
    eng.run()
    eng.sync()
    assert [len(eng.hops(ch)) for ch in chans] == [0] * 5
    pos += 1000
    while pos < len(streams[0]):
        for s, ch in zip(streams, chans):
            eng.push(ch, s[pos:pos + 12000])
        pos += 12000
        eng.run()
    eng.flush()
    for k, ch in enumerate(chans):
        h = np.concatenate(got[k] + [eng.hops(ch)])
        assert _same(h, refs[k][1]), 'channel %d hop records differ' % k
    eng.close()


@pytest.fixture(scope='module')
def seventy(cpu_libs):
    """The streams and push sizes of test_gpu_parity's 70-channel test."""
    nch = 70
    rng = np.random.default_rng(3)
    streams = [tl.synth(seconds=6.0, seed=0xAE60 + k, carrier=float(rng.uniform(11900, 12100)),
                        ebn0=float(rng.uniform(9, 14)), phase0=float(rng.uniform(0, 6.28)))
               for k in range(nch)]
    chunks = [int(rng.choice([1000, 4096, 12000, 30000])) for _ in range(nch)]
    return streams, chunks, _oracles(streams)


@pytest.mark.parametrize('grid', [3, 1])
def test_many_channels_per_workgroup(engine_lib, seventy, monkeypatch, grid):
    """70 channels out of step on 3 workgroups (24, 23 and 23 iterations) and
    on one (70 iterations: more than the 64 channels of one batch scan)."""
    import aero_engine as ae
    monkeypatch.setenv('AERO_COARSE_GRID', str(grid))
    streams, chunks, refs = seventy
    eng, chans = _run(ae, streams, chunks, ae.F_TRACE_SOFT)
    for k in range(len(streams)):
        assert np.array_equal(eng.softbits(chans[k]), refs[k][0]), 'channel %d soft bits differ' % k
        assert eng.items(chans[k]) == refs[k][2], 'channel %d items differ' % k
    eng.close()
