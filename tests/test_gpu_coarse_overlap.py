"""The persistent coarse kernel's overlapped head (coarse.hip, coarse_lds.h).

A due channel that follows another in its workgroup's batch has its head run
under that channel's tail: its ring words go into an LDS image behind ylds
(over the rest of lds, s_tw and a spare) while |X| is computed, the table
gathers go out under the log10 loop, s_tw is written again before the fold's
barrier, and the channel starts with the mix, without the plain head's two
barriers.  AERO_COARSE_OVERLAP=0 gives every channel the plain head.

Nothing may change by a bit: hop records (the ring image and its fix-up,
zero_before, the fold's argmax and the hop control behind them), soft bits,
items and the final smoothed spectrum y (aero_channel_coarse_y) equal the CPU
oracle's with the overlap on and off, in every adjacency of overlapped and
plain heads, across a batch boundary, for the C channel's instance and with
both instances in one engine.  (Hop records alone do not pin the y history
down: they hold the argmax of its fold.  y after every hop, on input that is
not a clean carrier, is tests/test_gpu_coarse_y.py.)"""
import concurrent.futures as cf

import numpy as np
import pytest

import aero_testlib as tl

pytestmark = pytest.mark.gpu

# the streams and push sizes of test_gpu_coarse_persistent.FIVE: 7020 and
# 15500 Hz retune (zero_before, yreset) behind a predecessor at grid 1, and
# the pushes of 4095/4096/4097 take the ring fix-up on a prefetched channel
FIVE = [(12037.5, 12.0, 1000), (12038.0, 12.0, 4095), (7020.0, 12.0, 4096), (15500.0, 12.0, 4097),
        (12040.0, 9.0, 30000)]
SECONDS = 8.0
C_THREE = ((12037.5, 12.0), (15500.0, 10.0), (9050.0, 8.0))  # test_c_channel_loops
HOP = 4096


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


@pytest.fixture(scope='module')
def c_three(cpu_libs):
    streams = [tl.synth_c(seconds=SECONDS, seed=0xC0B0 + k, carrier=f, ebn0=eb) for k, (f, eb) in enumerate(C_THREE)]
    return streams, _oracles(streams, 8400)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _env(mp, grid, overlap):
    mp.setenv('AERO_COARSE_GRID', str(grid))
    mp.setenv('AERO_COARSE_OVERLAP', str(overlap))


def _run_rounds(ae, streams, rounds, bitrate=10500):
    """rounds: per run() the number of samples pushed to each channel."""
    eng = ae.Engine(max_channels=len(streams), flags=ae.F_TRACE_SOFT | ae.F_TRACE_HOPS)
    chans = [eng.open_channel(bitrate, 48000) for _ in streams]
    pos = [0] * len(streams)
    for sizes in rounds:
        for k, (s, ch) in enumerate(zip(streams, chans)):
            if sizes[k] and pos[k] < len(s):
                eng.push(ch, s[pos[k]:pos[k] + sizes[k]])
                pos[k] += sizes[k]
        eng.run()
    assert all(p >= len(s) for p, s in zip(pos, streams)), 'the schedule pushes every stream to its end'
    eng.flush()
    return eng, chans


def _chunk_rounds(streams, chunks):
    """Every stream in its own chunk size, one run() per round, to the end."""
    n = max((len(s) + c - 1) // c for s, c in zip(streams, chunks))
    return [list(chunks)] * n


def _check(eng, chans, refs, what, units=False):
    for k, (ch, (rsb, rh, rit, ry)) in enumerate(zip(chans, refs)):
        assert _same(eng.hops(ch), rh), '%s: channel %d hop records differ' % (what, k)
        first, y = eng.channel_coarse_y(ch)
        assert _same(y, ry[first:first + len(y)]), '%s: channel %d final y differs' % (what, k)
        assert np.array_equal(eng.softbits(ch), rsb), '%s: channel %d soft bits differ' % (what, k)
        if units:
            assert np.array_equal(eng.c_units(ch), rit), '%s: channel %d Call_progress SUs differ' % (what, k)
        else:
            assert eng.items(ch) == rit, '%s: channel %d items differ' % (what, k)


@pytest.mark.parametrize('overlap', [1, 0])
@pytest.mark.parametrize('grid', [1, 2])
def test_on_off_oracle(engine_lib, five, monkeypatch, grid, overlap):
    import aero_engine as ae
    streams, refs = five
    assert len(refs[0][0]) > 1000 and refs[0][2], 'oracle did not lock on the plain channel'
    for k in (2, 3):  # the retunes happened: the centre frequency moved
        assert len(np.unique(refs[k][1][:, 3])) > 1, 'channel %d never retuned' % k
    _env(monkeypatch, grid, overlap)
    eng, chans = _run_rounds(ae, streams, _chunk_rounds(streams, [c[2] for c in FIVE]))
    for rh in (r[1] for r in refs):
        assert len(rh) >= int(SECONDS * 48000) // HOP - 1
    _check(eng, chans, refs, 'grid %d overlap %d' % (grid, overlap))
    eng.close()


# which of six channels have a hop due in one run(), as sets of channel numbers
PATTERNS = {'all': {0, 1, 2, 3, 4, 5}, 'first': {0}, 'last': {5}, 'first and last': {0, 5}, 'neighbours': {2, 3},
            'none': set(), 'every other': {0, 2, 4}}
DUE_SECONDS = 3.5


def _due_schedule(nsamp):
    """Rounds that walk through PATTERNS again and again: a channel in the
    round's pattern gets one hop's worth of samples (exactly one hop sample
    more is then pushed and that hop is due), the others none; the "none"
    round gives everyone 100 samples, which crosses no hop boundary.  When the
    busiest channel's stream is spent the rest is pushed 12000 at a time."""
    rounds, cum = [], [0] * 6
    names = list(PATTERNS)
    while max(cum) + HOP <= nsamp:
        for name in names:
            sizes = [100] * 6 if name == 'none' else [HOP if k in PATTERNS[name] else 0 for k in range(6)]
            if max(c + s for c, s in zip(cum, sizes)) > nsamp:
                break
            rounds.append(sizes)
            cum = [c + s for c, s in zip(cum, sizes)]
    while min(cum) < nsamp:
        sizes = [min(12000, nsamp - c) for c in cum]
        rounds.append(sizes)
        cum = [c + s for c, s in zip(cum, sizes)]
    return rounds


def _due_sets(rounds):
    """From the pushed sample counts alone: hop h of a channel is due in the
    run() after the push that brings its count to 4096 (h + 1) or more."""
    cum, out = [0] * 6, []
    for sizes in rounds:
        new = [c + s for c, s in zip(cum, sizes)]
        crossed = [n // HOP - c // HOP for c, n in zip(cum, new)]
        out.append((frozenset(k for k in range(6) if crossed[k]), max(crossed)))
        cum = new
    return out


@pytest.fixture(scope='module')
def six(cpu_libs):
    streams = [tl.synth(seconds=DUE_SECONDS, seed=0xC0D0 + k, carrier=12000.0 + 15.0 * k, ebn0=11.0 + 0.5 * k)
               for k in range(6)]
    return streams, _oracles(streams)


def test_due_patterns(engine_lib, six, monkeypatch):
    import aero_engine as ae
    streams, refs = six
    rounds = _due_schedule(len(streams[0]))
    seen = _due_sets(rounds)
    single = [s for s, most in seen if most <= 1]  # one coarse launch, this due set
    for name, want in PATTERNS.items():
        assert frozenset(want) in single, 'the schedule never has the due set "%s"' % name
    _env(monkeypatch, 1, 1)
    eng, chans = _run_rounds(ae, streams, rounds)
    for rh in (r[1] for r in refs):
        assert len(rh) >= int(DUE_SECONDS * 48000) // HOP - 1
    _check(eng, chans, refs, 'due patterns')
    eng.close()


@pytest.fixture(scope='module')
def sixty_six(cpu_libs):
    rng = np.random.default_rng(9)
    streams = [tl.synth(seconds=1.5, seed=0xC0E0 + k, carrier=float(rng.uniform(11900, 12100)),
                        ebn0=float(rng.uniform(9, 14)), phase0=float(rng.uniform(0, 6.28))) for k in range(66)]
    return streams, _oracles(streams)


def test_batch_boundary(engine_lib, sixty_six, monkeypatch):
    """66 channels in step on one workgroup: 63 overlapped heads, then
    channels 64 and 65 start a new batch with a plain head."""
    import aero_engine as ae
    streams, refs = sixty_six
    _env(monkeypatch, 1, 1)
    eng, chans = _run_rounds(ae, streams, _chunk_rounds(streams, [12000] * 66))
    for k, (ch, (rsb, rh, _, ry)) in enumerate(zip(chans, refs)):
        assert len(rh) >= int(1.5 * 48000) // HOP - 1
        assert _same(eng.hops(ch), rh), 'channel %d hop records differ' % k
        assert np.array_equal(eng.softbits(ch), rsb), 'channel %d soft bits differ' % k
        first, y = eng.channel_coarse_y(ch)
        assert _same(y, ry[first:first + len(y)]), 'channel %d final y differs' % k
    eng.close()


@pytest.mark.parametrize('overlap', [1, 0])
def test_c_channel(engine_lib, c_three, monkeypatch, overlap):
    import aero_engine as ae
    streams, refs = c_three
    _env(monkeypatch, 1, overlap)
    eng, chans = _run_rounds(ae, streams, _chunk_rounds(streams, [12000] * 3), bitrate=8400)
    assert all(len(r[1]) > 80 for r in refs)
    _check(eng, chans, refs, 'C channel overlap %d' % overlap, units=True)
    eng.close()


def test_mixed_engine(engine_lib, five, c_three, monkeypatch):
    """An OQPSK group and a C-channel group in one engine, both on one
    workgroup: each kernel instance has its own image map and log table, and
    writes s_tw again for itself."""
    import aero_engine as ae
    (so, ro), (sc, rc) = five, c_three
    so, ro, sc, rc = so[:3], ro[:3], sc[:2], rc[:2]
    _env(monkeypatch, 1, 1)
    eng = ae.Engine(max_channels=5, flags=ae.F_TRACE_SOFT | ae.F_TRACE_HOPS)
    co = [eng.open_channel(10500, 48000) for _ in so]
    cc = [eng.open_channel(8400, 48000) for _ in sc]
    n = max(len(s) for s in so + sc)
    for pos in range(0, n, 12000):
        for s, ch in zip(so + sc, co + cc):
            if pos < len(s):
                eng.push(ch, s[pos:pos + 12000])
        eng.run()
    eng.flush()
    _check(eng, co, ro, 'mixed engine, OQPSK')
    _check(eng, cc, rc, 'mixed engine, C channel', units=True)
    eng.close()
