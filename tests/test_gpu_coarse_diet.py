"""The coarse kernel with its trimmed instruction stream (coarse.hip): log10
of max(|X|, 1) by aero_log10_ge1_tab behind one wave-uniform test, the mix
without the zero_before test while the whole snapshot is live, the |X| range
test over the stored registers only, aero_hypot_nr's larger and smaller by
v_max_f64 / v_min_f64.  Nothing may change by a bit.

One engine of three channels per case, fed the streams of
tests/coarse_diet_inputs.py one hop per run() (silence then a carrier,
+-1 LSB noise, a carrier the hunter has to find, a carrier the AFC pulls in;
tests/test_coarse_near1_inputs.py shows on the CPU what they reach: hops of
nothing but near-1 bins, threads with 5 and more of them, waves with none,
zero_before inside the snapshot and on its first element).  After every run()
each channel's y (aero_channel_coarse_y) equals the oracle's by bit pattern,
and so do the hop counts and hop records.  The 16384-point kinds run on one and
two workgroups with the overlapped head on and off: on one workgroup the
engine's first channel takes the plain head, the next ones the overlapped
head, the last one has no successor; the two trios put the silent stream first
and last and a live one in every position, and once the shorter streams are
spent the due sets shrink to two channels and to one.  The oracle's walk of
each stream is computed once and shared by every case."""
import numpy as np
import pytest

import aero_testlib as tl  # noqa: F401  (puts the package on sys.path)
import coarse_diet_inputs as di
import coarse_inputs as ci

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _compare(ae, mode, trio, what):
    bitrate, fs, hop, nfft, _ = ci.MODES[mode]
    lo, hi = ci.KEPT[nfft]
    names = di.TRIOS[trio]
    streams = [di.stream(mode, n) for n in names]
    walks = [di.walk(mode, n) for n in names]
    eng = ae.Engine(max_channels=len(streams), flags=ae.F_TRACE_HOPS)
    try:
        chans = [eng.open_channel(bitrate, fs) for _ in streams]
        got = [np.zeros((0, 6)) for _ in streams]
        for r in range(max(len(w) for w in walks)):
            for c, s in enumerate(streams):
                if r < len(walks[c]):
                    eng.push(chans[c], s[r * hop:(r + 1) * hop], fs)
            eng.run()
            eng.sync()
            for c, w in enumerate(walks):
                _, ry, rh = w[min(r, len(w) - 1)]
                where = '%s, %s (channel %d) after run %d' % (what, names[c], c, r)
                got[c] = np.concatenate([got[c], eng.hops(chans[c]).reshape(-1, 6)])
                assert len(got[c]) == len(rh), '%s: hop counts %d (engine) %d (oracle)' % (where, len(got[c]), len(rh))
                first, y = eng.channel_coarse_y(chans[c])
                assert (first, len(y)) == (lo, hi - lo + 1), where
                bad = np.flatnonzero(_bits(y) != _bits(ry))
                assert not len(bad), '%s: %d of %d y bins differ, first bin %d: %r (engine) %r (oracle)' % (
                    where, len(bad), len(y), lo + bad[0], y[bad[0]], ry[bad[0]])
                assert np.array_equal(_bits(got[c]), _bits(rh)), '%s: hop records differ' % where
    finally:
        eng.close()


@pytest.mark.parametrize('trio', sorted(di.TRIOS))
@pytest.mark.parametrize('grid,overlap', [(1, 1), (1, 0), (2, 1), (2, 0)])
@pytest.mark.parametrize('mode', ['oqpsk10500@48000', 'c8400@48000'])
def test_y_and_hops_16384(engine_lib, monkeypatch, mode, grid, overlap, trio):
    import aero_engine as ae
    monkeypatch.setenv('AERO_COARSE_GRID', str(grid))
    monkeypatch.setenv('AERO_COARSE_OVERLAP', str(overlap))
    _compare(ae, mode, trio, '%s grid %d overlap %d trio %s' % (mode, grid, overlap, trio))


@pytest.mark.parametrize('trio', sorted(di.TRIOS))
def test_y_and_hops_msk(engine_lib, trio):
    import aero_engine as ae
    _compare(ae, 'msk600@12000', trio, 'msk600@12000 trio %s' % trio)


def test_device_log10_ge1_matches_host(engine_lib):
    """aero_log10_ge1 on the device (as the kernel calls it, aero_log10_ge1_w)
    against the host build, on the CPU test's boundary set
    (tests/test_math_log10_ge1.py) and on log-uniform arguments."""
    import aero_engine as ae
    import mathhost
    eng = ae.Engine(max_channels=1)
    try:
        rng = np.random.default_rng(0x10611)
        for x in (di.boundary_set(), np.exp2(rng.uniform(0.0, 1023.0, 400_000)),
                  (1.0 + rng.uniform(0.0, 0.13, 100_000)) * np.exp2(rng.integers(0, 64, 100_000))):
            dev = eng.device_math('log10_ge1', x)
            host = di.host_log10_ge1(x)
            bad = np.flatnonzero(_bits(dev) != _bits(host))
            assert not len(bad), (len(bad), x[bad[:4]], dev[bad[:4]], host[bad[:4]])
            assert np.array_equal(_bits(dev), _bits(eng.device_math('log10', x)))
        # waves with an infinite lane take the general function, and give its result in every lane
        x = np.exp2(rng.uniform(0.0, 1023.0, 1 << 16))
        x[5::193] = np.inf
        dev = eng.device_math('log10_ge1', x)
        assert np.array_equal(_bits(dev), _bits(mathhost.glibc('log10', x))) and np.isinf(dev[5])
    finally:
        eng.close()
