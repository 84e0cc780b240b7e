"""What the streams of tests/test_gpu_coarse_diet.py reach in the coarse
kernel's log10 loop and mix, shown with the oracle alone (oracle_coarse_absx,
hop records), one hop per message as the GPU test pushes them.

log10's argument is max(|X|, 1); log takes its polynomial around 1 when the
argument's mantissa is below 1 + 0x1.09p-4 and its table otherwise
(aero_log10_ge1_tab, aero_math.h), per lane, so what a wave executes depends
on which of its lanes hold such a near-1 bin.  Thread t of FT = nfft / 16
works on the kept bins k = t, t + FT, ...; a wave is 64 consecutive t.  The
streams hold every composition a wave can meet, and those that a kernel which
runs the polynomial apart from the loop, for the lanes that need it, can get
wrong ("The coarse kernel's non-transform instructions": measured,
slower, not kept): a hop in which every bin is a near-1 one (silence: every
argument exactly 1.0) and live hops after it on the same channel; a thread with
at least 5 such bins in one hop (the 8192-point kinds give a thread 3 or 4
bins: there, one with at least 3 in a live hop); lanes of one wave with
different numbers of them; and a wave's iteration, 64 aligned bins, with none.

The mix looks at an element's sample number only when zero_before lies inside
the snapshot, s0 < zero_before.  zero_before is the sample after a hop in
which the centre frequency moved (hop_control, coarse.hip), s0 the sample of
the snapshot's first element; both are multiples of the hop, so
zero_before - s0 takes the values nfft - hop, ..., hop (inside: the mix with
the test), 0 (the first hop without it again) and below, and never 1: asserted
here as it is, with the hop on either side of the switch (hop and 0).

These are conditions on the inputs: if one fails, the stream is changed, not
the condition."""
import numpy as np
import pytest

import coarse_diet_inputs as di
import coarse_inputs as ci

NAMES = ('silence_carrier', 'lsb_noise', 'hunting', 'locked')


def _threads(near, ft):
    """Per thread the number of near-1 bins of one hop."""
    n = len(near)
    return np.concatenate([near, np.zeros((-n) % ft, dtype=bool)]).reshape(-1, ft).sum(0)


def _clean_waves(near):
    """Aligned runs of 64 bins (one wave's iteration) with no near-1 bin."""
    n = len(near) // 64 * 64
    return int((~near[:n].reshape(-1, 64).any(1)).sum())


def _live(absx):
    return (absx > 1.0).mean() > 0.5


@pytest.mark.parametrize('mode', di.MODES)
def test_trios_use_the_streams(mode, cpu_libs):
    assert sorted(set(sum(di.TRIOS.values(), ()))) == sorted(NAMES)
    hop = ci.MODES[mode][2]
    for name in NAMES:
        s = di.stream(mode, name)
        assert s.dtype == np.int16 and len(s) % hop == ci.TAIL and len(s) // hop >= 17


@pytest.mark.parametrize('mode', di.MODES)
def test_silence_then_signal(mode, cpu_libs):
    w = [r for r in di.walk(mode, 'silence_carrier') if r[0] is not None]
    ones = [bool((np.maximum(a, 1.0) == 1.0).all()) for a, _, _ in w]
    assert ones[0] and di.near1(w[0][0]).all(), 'silence: every argument exactly 1.0, every bin a near-1 one'
    k = ones.index(False)
    assert k >= ci.STEP_HOP[mode] and all(ones[:k]), 'silent until the hunter has stepped'
    live = [i for i in range(k, len(w)) if _live(w[i][0])]
    assert live, 'a live hop after the silence'
    near = di.near1(w[live[-1]][0])
    assert 0.03 < near.mean() < 0.2, 'about 9 %% of a live hop are near-1 bins: %.3f' % near.mean()


@pytest.mark.parametrize('mode', di.MODES)
def test_full_threads_and_clean_waves(mode, cpu_libs):
    nfft = ci.MODES[mode][3]
    ft = nfft // 16
    ylen = ci.KEPT[nfft][1] - ci.KEPT[nfft][0] + 1
    want = 5 if (ylen + ft - 1) // ft >= 11 else 3
    full, clean, mixed = 0, 0, 0
    for name in NAMES:
        for absx, _, _ in di.walk(mode, name):
            if absx is None or not _live(absx):
                continue
            near = di.near1(absx)
            per = _threads(near, ft)
            full += int(per.max() >= want)
            clean += int(_clean_waves(near) > 0)
            # one wave whose lanes have different numbers of near-1 bins
            mixed += int(len(set(per[:64])) > 1)
    assert full, 'a live hop in which some thread has at least %d near-1 bins' % want
    assert clean, "a live hop with a wave's iteration (64 aligned bins) that has none"
    assert mixed, 'lanes of one wave with different numbers of near-1 bins'


@pytest.mark.parametrize('mode', di.MODES)
def test_lsb_noise_mixes_exact_ones_and_live_bins(mode, cpu_libs):
    hit = False
    for absx, _, _ in di.walk(mode, 'lsb_noise'):
        if absx is not None:
            a = np.maximum(absx, 1.0)
            hit = hit or bool((a == 1.0).any() and (a > 1.0).any() and (~di.near1(absx)).any())
    assert hit, 'arguments of exactly 1.0 beside table-path ones in one hop'


@pytest.mark.parametrize('mode', di.MODES)
def test_zero_before_around_a_centre_step(mode, cpu_libs):
    hop, nfft = ci.MODES[mode][2:4]
    seen = set()
    for name in NAMES:
        h = di.walk(mode, name)[-1][2]
        nk, mcf = h[:, 0], h[:, 3]
        assert np.array_equal(nk, hop * (np.arange(len(h)) + 1.0) - 1.0)
        zb = None  # zero_before as hop i reads it: set by the last hop before it that moved the centre
        for i in range(1, len(h)):
            if mcf[i - 1] != (mcf[i - 2] if i >= 2 else mcf[i - 1]):
                zb = int(nk[i - 1]) + 1
            if zb is not None:
                s0 = int(nk[i]) - (nfft - 1)
                assert (zb - s0) % hop == 0, 'zero_before and s0 are multiples of the hop'
                seen.add(zb - s0)
    assert {nfft - hop, hop, 0} <= seen, sorted(seen)  # strictly inside; its last hop; zero_before == s0
    assert min(seen) < 0 and 1 not in seen
