"""The coarse estimator's real output, the smoothed spectrum y, bit for bit.

Hop records show the argmax of the folded y only, which a clean carrier holds
against any small error.  Here every class of tests/coarse_inputs.py (silence,
full scale, -32768, +-1 LSB noise, one sample, an exact-bin tone, noise, fold
peaks on both edges of the search range, silence then a carrier, an AFC
reset followed by silence) is a channel of one engine per mode, and after
EVERY run() each channel's y (aero_channel_coarse_y: the bins the engine
keeps) equals the oracle's slice by bit pattern, the hop counts of both equal
pushed // HOP, and the hop records so far are equal.  Two schedules: one hop
per run(), and HOP - 1, HOP + 1, 3 HOP + 7, 1, 2 HOP - 8, ...  The
16384-point kinds run on one workgroup with the overlapped head on and off
(every class is then a plain head and a successor under its neighbour's tail;
silence and full scale are neighbours), and once on two workgroups.
tests/test_coarse_inputs.py shows which paths the classes reach."""
import functools

import numpy as np
import pytest

import aero_testlib as tl  # noqa: F401  (puts the package on sys.path)
import coarse_inputs as ci

pytestmark = pytest.mark.gpu

SCHEDULES = ('hop', 'ragged')


def _sizes(schedule, hop):
    return [hop] if schedule == 'hop' else [hop - 1, hop + 1, 3 * hop + 7, 1, 2 * hop - 8]


def _rounds(mode, schedule):
    """Per run() and channel the [start, stop) of the samples pushed (None: the stream is spent)."""
    hop = ci.MODES[mode][2]
    lens = [len(s) for _, s in ci.streams(mode)]
    sizes, pos, out, k = _sizes(schedule, hop), [0] * len(lens), [], 0
    while any(p < n for p, n in zip(pos, lens)):
        step = sizes[k % len(sizes)]
        k += 1
        out.append([(p, min(n, p + step)) if p < n else None for p, n in zip(pos, lens)])
        pos = [min(n, p + step) for p, n in zip(pos, lens)]
    return out


@functools.lru_cache(maxsize=None)
def _reference(mode, schedule):
    """The oracle at every checkpoint: per run() and channel (samples pushed,
    y of the kept bins, hop records so far).  Computed once per mode and
    schedule, shared by the engine configurations, never changed."""
    nfft = ci.MODES[mode][3]
    lo, hi = ci.KEPT[nfft]
    streams = [s for _, s in ci.streams(mode)]
    orc = [ci.oracle(mode) for _ in streams]
    pushed, out = [0] * len(streams), []
    for rnd in _rounds(mode, schedule):
        row = []
        for c, span in enumerate(rnd):
            if span:
                ci.push(orc[c], mode, streams[c][span[0]:span[1]])
                pushed[c] = span[1]
            y = orc[c].coarse_y()[lo:hi + 1].copy()
            h = orc[c].hops().copy()
            y.setflags(write=False)
            h.setflags(write=False)
            row.append((pushed[c], y, h))
        out.append(row)
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _compare(ae, mode, schedule, what):
    bitrate, fs, hop, nfft, _ = ci.MODES[mode]
    lo, hi = ci.KEPT[nfft]
    names = [n for n, _ in ci.streams(mode)]
    streams = [s for _, s in ci.streams(mode)]
    ref = _reference(mode, schedule)
    eng = ae.Engine(max_channels=len(streams), flags=ae.F_TRACE_HOPS)
    try:
        chans = [eng.open_channel(bitrate, fs) for _ in streams]
        got_hops = [np.zeros((0, 6)) for _ in streams]
        for r, (rnd, row) in enumerate(zip(_rounds(mode, schedule), ref)):
            for c, span in enumerate(rnd):
                if span:
                    eng.push(chans[c], streams[c][span[0]:span[1]], fs)
            eng.run()
            eng.sync()
            for c, (pushed, ry, rh) in enumerate(row):  # every channel at every checkpoint
                where = '%s %s, %s after run %d (%d samples)' % (what, schedule, names[c], r, pushed)
                got_hops[c] = np.concatenate([got_hops[c], eng.hops(chans[c]).reshape(-1, 6)])
                assert len(got_hops[c]) == len(rh) == pushed // hop, '%s: hop counts %d (engine) %d (oracle)' % (
                    where, len(got_hops[c]), len(rh))
                first, y = eng.channel_coarse_y(chans[c])
                assert (first, len(y)) == (lo, hi - lo + 1), where
                bad = np.flatnonzero(_bits(y) != _bits(ry))
                assert not len(bad), '%s: %d of %d y bins differ, first bin %d: %r (engine) %r (oracle)' % (
                    where, len(bad), len(y), lo + bad[0], y[bad[0]], ry[bad[0]])
                assert np.array_equal(_bits(got_hops[c]), _bits(rh)), '%s: hop records differ' % where
    finally:
        eng.close()


@pytest.mark.parametrize('schedule', SCHEDULES)
@pytest.mark.parametrize('grid,overlap', [(1, 1), (1, 0), (2, 1)])
@pytest.mark.parametrize('mode', ['oqpsk10500@48000', 'c8400@48000'])
def test_y_16384(engine_lib, monkeypatch, mode, grid, overlap, schedule):
    import aero_engine as ae
    monkeypatch.setenv('AERO_COARSE_GRID', str(grid))
    monkeypatch.setenv('AERO_COARSE_OVERLAP', str(overlap))
    _compare(ae, mode, schedule, '%s grid %d overlap %d' % (mode, grid, overlap))


@pytest.mark.parametrize('schedule', SCHEDULES)
@pytest.mark.parametrize('mode', [m for m in ci.MODES if m.startswith('msk')])
def test_y_msk(engine_lib, mode, schedule):
    import aero_engine as ae
    _compare(ae, mode, schedule, mode)


def test_burst_channel_has_no_y(engine_lib):
    import aero_engine as ae
    eng = ae.Engine(max_channels=2)
    try:
        ch = eng.open_channel(10500, 48000, burst=True)
        with pytest.raises(ae.AeroError) as ei:
            eng.channel_coarse_y(ch)
        assert ei.value.rc == ae.AERO_E_INVALID
    finally:
        eng.close()
