"""What the streams of tests/coarse_inputs.py reach in the coarse estimator,
shown with the reference alone (oracle_coarse_absx, oracle_coarse_y, hop
records), one hop per message as tests/test_gpu_coarse_y.py's first schedule
pushes them: an all-zero |X|; |X| on both sides of the fmax(|X|, 1) floor in
one record; fold sums that all tie, so that the default / the first index
decides; y of exactly 20 after bigchange(); a hunter step that moves the
centre; a fold peak in the first and in the last bin of the search range.
These are conditions on the inputs: if one fails, the class is changed, not
the condition."""
import numpy as np
import pytest

import coarse_inputs as ci

MODES = list(ci.MODES)


@pytest.fixture(scope='module')
def walks(cpu_libs):
    """(mode, class) -> (per hop |X| of the kept bins, per hop y, hop records, hunter steps), computed once."""
    cache = {}

    def get(mode, name):
        if (mode, name) not in cache:
            _, _, hop, nfft, _ = ci.MODES[mode]
            lo, hi = ci.KEPT[nfft]
            pcm = dict(ci.streams(mode))[name]
            o = ci.oracle(mode)
            absx, ys = [], []
            for k in range(0, len(pcm), hop):
                ci.push(o, mode, pcm[k:k + hop])
                if len(pcm) - k >= hop:  # a whole hop: the estimator ran
                    absx.append(o.coarse_absx()[lo:hi + 1])
                    ys.append(o.coarse_y())
            h = o.hops()
            assert len(h) == len(absx) == len(pcm) // hop and len(pcm) % hop == ci.TAIL
            cache[mode, name] = (absx, ys, h, o.events()[1])
        return cache[mode, name]
    return get


@pytest.mark.parametrize('mode', MODES)
def test_class_list_and_lengths(mode, cpu_libs):
    _, _, hop, _, _ = ci.MODES[mode]
    sil, got = ci.silent_hops(mode), dict(ci.streams(mode))
    has_reset = mode in ('oqpsk10500@48000', 'c8400@48000')
    assert list(got) == [n for n in ci.ORDER if has_reset or n != 'reset_silence']
    assert [n for n, _ in ci.streams(mode)][:2] == ['silence', 'square']  # neighbours
    for name in ('silence', 'one_sample', 'lsb_noise'):
        assert len(got[name]) == sil * hop + ci.TAIL
    for name in ('square', 'const_min', 'tone', 'noise'):
        assert len(got[name]) == ci.HOPS * hop + ci.TAIL
    assert len(got['silence_carrier']) == (sil + ci.HOPS) * hop + ci.TAIL
    assert not got['silence'].any() and np.count_nonzero(got['one_sample']) == 1
    assert set(np.unique(got['lsb_noise'])) == {-1, 0, 1}
    assert set(np.unique(got['square'])) == {-32768, 32767} and set(np.unique(got['const_min'])) == {-32768}
    assert all(v.dtype == np.int16 for v in got.values())
    if not has_reset:  # the MSK demodulator's AFC branch needs dcd, which nothing sets
        assert ci.reset_stream(mode) == (None, None)


@pytest.mark.parametrize('mode', MODES)
def test_silence_zero_spectrum_ties_and_hunter_step(mode, walks):
    absx, ys, h, steps = walks(mode, 'silence')
    nfft = ci.MODES[mode][3]
    lo, hi = ci.KEPT[nfft]
    assert all(not a.any() for a in absx), 'an all-zero |X| in every hop'
    for y in ys:  # every fold sum ties: the search keeps its default, the centre bin
        assert (y[lo:hi + 1] == y[lo]).all()
    assert not h[:, 1].any()
    k = ci.STEP_HOP[mode]  # the first hunter step, and the centre moves with it
    assert len(steps) == 1 and (h[:k - 1, 3] == h[0, 3]).all() and h[k - 1, 3] == steps[0] != h[0, 3]


@pytest.mark.parametrize('mode', MODES)
def test_one_sample_and_lsb_noise_straddle_the_floor(mode, walks):
    absx, _, _, _ = walks(mode, 'lsb_noise')
    both = [bool((a < 1).any() and (a > 1).any()) for a in absx]
    assert any(both), '|X| < 1 and |X| > 1 inside the kept bins of one record'
    absx, ys, _, _ = walks(mode, 'one_sample')
    live = [bool(a.any()) for a in absx]
    assert any(live) and not live[-1], 'the sample passes through the snapshot and leaves it'
    assert ys[-1].max() > 0, 'and y still decays from it'


@pytest.mark.parametrize('mode', MODES)
def test_full_scale_classes(mode, walks):
    for name in ('square', 'const_min'):
        absx, ys, _, _ = walks(mode, name)
        assert max(a.max() for a in absx) > 1e6 and np.isfinite(ys[-1]).all()


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('edge', ['lo', 'hi'])
def test_edge_peaks(mode, edge, walks):
    """zmaxloc = N/2 - 2 est nfft / fs falls on ILO / on IHI - 1 in some hop."""
    _, fs, _, nfft, _ = ci.MODES[mode]
    ilo, ihi, _ = ci.fold_range(mode)
    _, _, h, _ = walks(mode, 'edge_' + edge)
    zmaxloc = nfft / 2 - 2 * h[:, 1] * nfft / fs
    assert (zmaxloc == (ilo if edge == 'lo' else ihi - 1)).any(), sorted(set(zmaxloc))


@pytest.mark.parametrize('mode', MODES)
def test_silence_then_carrier_takes_the_step_first(mode, walks):
    _, _, h, steps = walks(mode, 'silence_carrier')
    assert len(steps) >= 1 and h[-1, 3] != h[0, 3]
    assert h[ci.silent_hops(mode):, 1].any(), 'the carrier is seen after the step'


@pytest.mark.parametrize('mode', ['oqpsk10500@48000', 'c8400@48000'])
def test_reset_then_ties_pick_the_first_bin(mode, walks):
    absx, ys, h, _ = walks(mode, 'reset_silence')
    r = ci.reset_stream(mode)[1]
    assert (ys[r - 1] == 20.0).all(), 'y is exactly 20 in every bin after bigchange()'
    assert not (ys[r - 2] == 20.0).all() and h[r - 1, 3] != h[r - 2, 3]  # the AFC moved the centre in that hop
    assert len(h) == r + ci.RESET_TAIL_HOPS
    for k in range(r, len(h)):  # silence into the cleared snapshot: y = 18, 16.2, ... in every bin
        assert not absx[k].any() and (ys[k] == ys[k][0]).all() and 0 < ys[k][0] < 20
    # emptyingcountdown holds the estimate at 0 for four hops; then, with every
    # fold sum equal, the first bin of the search range
    assert not h[r:-1, 1].any() and h[-1, 1] == ci.edge_est(mode, 'lo')
