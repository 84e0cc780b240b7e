"""The continuous demodulators on adversarial PCM, bit for bit against the oracle.

Every class of tests/cont_inputs.py (silence, full scale, -32768, one and two
samples, 1-LSB noise, noise, tones, the tone that drives the rotation argument
furthest, the synthetic carrier plain, clipped, at +-4 LSB, negated, from
sample 0, behind a second of zeros, cut off into silence, full scale and
noise, gated on and off, and overlapping itself) is a channel of one engine
per mode (OQPSK 10500, C 8400, MSK 600 at 12, 22.05 and 48 kHz, MSK 1200 at
24 kHz).  tests/test_cont_inputs.py shows which fast-path limits they reach.

Flags: F_TRACE_PT | F_TRACE_SOFT | F_TRACE_HOPS | F_TRACE_FRAMES and
F_TRACE_BLOCKS (without it the engine keeps no Viterbi blocks to compare),
with the mode's DCD timer (F_DCD_TICK for OQPSK, F_DCD_TICK_CONT for MSK and
C) off and on.  Compared per channel: pt and hop records by f64 bit pattern,
soft bits, Viterbi blocks, frames, ACARS items, C: Call_progress SUs and voice
frames; after flush() the DataCarrierDetect changes, the hunter's steps and
their centres.

When.  A run() without flush advances a continuous OQPSK or MSK channel to
its last whole hop: with P samples pushed it has the hop records of P // HOP
hops and has demodulated the samples below the hop sample of the last one,
[0, HOP (P // HOP) - 1) (the segment contract at the head of
demod_oqpsk.hip), and a pass's Viterbi may run in the next pass.  So after
EVERY run() + sync() each trace so far must be a prefix of the oracle's final
trace, the hop count must equal P // HOP, and pt and the soft bits must be at
least as long as the oracle's after HOP (P // HOP) - 1 samples (the OQPSK and
MSK oracles are chunk-invariant, so that is a second reference, fed hop by
hop).  A C channel demodulates every whole message it was given (the same
contract on prefiltered samples: its segment ends at the prefiltered end),
so its bound is the oracle's length after the same messages.  After flush() +
sync() everything is equal, the 37-sample tail included.

Layouts.  mixed: every class once, in ORDER; all three schedules, both kernel
shapes.  In a one-lane kernel the 20 channels are one wave, so one silent lane
sends all lanes through the general libm forms.  In a 16-lane kernel a wave
holds 4 channels, ORDER falls into 5 waves, and only the first two hold a
silent class (silence, square, synth, const_min; one_sample, lsb_noise, clip,
two_samples).  beside_silence is the layout for the other twelve classes in
those kernels: four waves of a silent class and three of them, so that tiny,
negated, lead0, late, overlap, the cut and gated carriers and tone_far decode
through the general forms there too.  homogeneous: every class fills __all units of its own (64
consecutive lanes of a one-lane kernel, 4 consecutive channels of a 16-lane
kernel; four classes per engine), so a class inside the fast ranges runs the
branch-free forms, and cut_silence, gated and one_sample run them up to
their limits.  two_waves: 70
channels of the one-lane OQPSK kernel and the C kernel, the second wave
partial and starting with other classes than the first."""
import concurrent.futures as cf
import functools

import numpy as np
import pytest

import aero_testlib as tl  # noqa: F401  (puts the package on sys.path)
import cont_inputs as xi

pytestmark = pytest.mark.gpu

MSK_MODES = [m for m in xi.MODES if xi.is_msk(m)]


def _traces(mode):
    """what is compared (the engine keeps no Viterbi blocks of a C channel)"""
    if xi.dims(mode)[0] == 8400:
        return ('pt', 'hops', 'soft', 'frames', 'items', 'c_units', 'voice')
    return ('pt', 'hops', 'soft', 'blocks', 'frames', 'items')


def _frozen(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _walk_class(mode, schedule, tick, pcm):
    """one oracle channel fed the schedule's messages: (final outputs, per
    run() the lengths of pt and the soft bits so far)"""
    o = xi.oracle(mode, tick)
    counts = []
    for grp in xi.runs(mode, len(pcm), schedule):
        for a, b in grp:
            o.push(pcm[a:b])
        counts.append((len(o.pt()), len(o.softbits())))
    return _frozen(xi.outputs(o)), tuple(counts)


def _bound_class(mode, tick, pcm):
    """[(pt, soft bits)] the oracle has delivered after HOP h - 1 samples, h = 0, 1, ..."""
    hop = xi.dims(mode)[2]
    o, out, p = xi.oracle(mode, tick), [(0, 0)], 0
    for h in range(1, len(pcm) // hop + 1):
        o.push(pcm[p:h * hop - 1])
        p = h * hop - 1
        out.append((len(o.pt()), len(o.softbits())))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _reference(mode, schedule, tick):
    """The oracle per class, fed the engine's messages.  Computed once per
    mode, schedule and tick, shared by every layout, never changed."""
    xi.oracle(mode, tick)  # the library is built and loaded before the threads start
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        futs = [ex.submit(_walk_class, mode, schedule, tick, pcm) for _, pcm in xi.streams(mode)]
        return tuple(f.result() for f in futs)


@functools.lru_cache(maxsize=None)
def _bounds(mode, tick):
    """the second reference (OQPSK, MSK): see _bound_class"""
    xi.oracle(mode, tick)
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        futs = [ex.submit(_bound_class, mode, tick, pcm) for _, pcm in xi.streams(mode)]
        return tuple(f.result() for f in futs)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _first_diff(got, ref, whole):
    """index of the first entry (row) of got that is not ref's; None if got is
    ref (whole) or a prefix of it"""
    n = min(len(got), len(ref))
    if isinstance(ref, np.ndarray):
        width = max(1, int(np.prod(ref.shape[1:])))
        g, r = _bits(got[:n]).reshape(n, width), _bits(ref[:n]).reshape(n, width)
        bad = np.flatnonzero((g != r).any(axis=1))
    else:
        bad = [k for k in range(n) if got[k] != ref[k]]
    if len(bad):
        return int(bad[0])
    if len(got) > len(ref) or (whole and len(got) < len(ref)):
        return n
    return None


def _show(seq, k):
    """entry k; f64 values in hex as well, so that a difference in the last bit shows"""
    if k >= len(seq):
        return 'nothing (%d entries)' % len(seq)
    if isinstance(seq, np.ndarray) and seq.dtype == np.float64:
        return '%r [%s]' % (seq[k].tolist(), ' '.join(float(v).hex() for v in seq[k]))
    return repr(seq[k])


def _take(eng, ch, traces):
    get = dict(pt=eng.pt, hops=eng.hops, soft=eng.softbits, blocks=eng.blocks, frames=eng.frames, items=eng.items,
               c_units=eng.c_units, voice=eng.voice)
    return {t: get[t](ch) for t in traces}


def _empty(traces):
    zero = dict(pt=np.zeros((0, 2)), hops=np.zeros((0, 6)), soft=np.zeros(0, np.uint8), blocks=np.zeros(0, np.uint8),
                frames=np.zeros(0, np.uint8), c_units=np.zeros((0, 12), np.uint8), items=[], voice=[])
    return {t: zero[t] for t in traces}


def _append(acc, new):
    for t in new:
        acc[t] = acc[t] + new[t] if isinstance(new[t], list) else np.concatenate([acc[t], new[t]])


def _flags(ae, mode, tick):
    timer = ae.F_DCD_TICK if xi.dims(mode)[0] == 10500 else ae.F_DCD_TICK_CONT
    return (ae.F_TRACE_PT | ae.F_TRACE_SOFT | ae.F_TRACE_HOPS | ae.F_TRACE_FRAMES | ae.F_TRACE_BLOCKS |
            (timer if tick else 0))


def _compare(ae, mode, schedule, tick, classes, every_run=True, layout='mixed'):
    """One engine whose channel j carries class classes[j]; every channel
    against the oracle after every run() (every_run) and after flush().
    Returns the engine's channel handles."""
    bitrate, fs, hop = xi.dims(mode)
    names = [n for n, _ in xi.streams(mode)]
    pcms = [p for _, p in xi.streams(mode)]
    ref = _reference(mode, schedule, tick)
    bounds = None if bitrate == 8400 else _bounds(mode, tick)
    traces = _traces(mode)
    plans = {k: xi.runs(mode, len(pcms[k]), schedule) for k in set(classes)}
    where = '%s %s %s%s' % (mode, layout, schedule, ' ticked' if tick else '')
    eng = ae.Engine(max_channels=len(classes), flags=_flags(ae, mode, tick))
    try:
        chans = [eng.open_channel(bitrate, fs) for _ in classes]
        acc = [_empty(traces) for _ in classes]
        pushed = [0] * len(classes)

        def check(r, what, whole):
            for j, k in enumerate(classes):
                final, counts = ref[k]
                _append(acc[j], _take(eng, chans[j], traces))
                for t in traces:
                    bad = _first_diff(acc[j][t], final[t], whole)
                    assert bad is None, '%s, %s (channel %d), %s %d: %s differ at %d: %s (engine) %s (oracle)' % (
                        where, names[k], j, what, r, t, bad, _show(acc[j][t], bad), _show(final[t], bad))
                if whole:
                    continue
                nh = pushed[j] // hop
                assert len(acc[j]['hops']) == nh, '%s, %s (channel %d), %s %d: %d hop records, %d samples pushed' % (
                    where, names[k], j, what, r, len(acc[j]['hops']), pushed[j])
                need = counts[min(r, len(counts) - 1)] if bounds is None else bounds[k][nh]
                for t, n in zip(('pt', 'soft'), need):
                    assert len(acc[j][t]) >= n, '%s, %s (channel %d), %s %d: %d of %s, the oracle has %d by then' % (
                        where, names[k], j, what, r, len(acc[j][t]), t, n)

        nruns = max(len(p) for p in plans.values())
        for r in range(nruns):
            depth = max(len(p[r]) for p in plans.values() if r < len(p))
            for m in range(depth):  # the channels' queued messages interleaved
                for j, k in enumerate(classes):
                    if r < len(plans[k]) and m < len(plans[k][r]):
                        a, b = plans[k][r][m]
                        eng.push(chans[j], pcms[k][a:b], fs)
                        pushed[j] = b
            eng.run()
            if every_run:
                eng.sync()
                check(r, 'after run', False)
        eng.flush()
        eng.sync()
        check(nruns, 'after flush, run', True)
        for j, k in enumerate(classes):
            final = ref[k][0]
            got = eng.channel_events(chans[j])
            want = (final['edges'], len(final['centres']), final['centres'][-8:])
            assert got == want, '%s, %s (channel %d): (DataCarrierDetect changes, hunter steps, last centres) %r ' \
                '(engine) %r (oracle)' % (where, names[k], j, got, want)
        return chans
    finally:
        eng.close()


ALL = list(range(len(xi.ORDER)))


# ------------------------------------------------------------------ mixed
@pytest.mark.parametrize('tick', [False, True], ids=['untimed', 'ticked'])
@pytest.mark.parametrize('schedule', xi.SCHEDULES)
def test_mixed_oqpsk(engine_lib, oqpsk_kernel, schedule, tick):
    import aero_engine as ae
    _compare(ae, 'oqpsk10500@48000', schedule, tick, ALL)


@pytest.mark.parametrize('tick', [False, True], ids=['untimed', 'ticked'])
@pytest.mark.parametrize('schedule', xi.SCHEDULES)
def test_mixed_c(engine_lib, schedule, tick):
    import aero_engine as ae
    _compare(ae, 'c8400@48000', schedule, tick, ALL)


@pytest.mark.parametrize('tick', [False, True], ids=['untimed', 'ticked'])
@pytest.mark.parametrize('schedule', xi.SCHEDULES)
@pytest.mark.parametrize('mode', MSK_MODES)
def test_mixed_msk(engine_lib, msk_kernel, mode, schedule, tick):
    import aero_engine as ae
    _compare(ae, mode, schedule, tick, ALL)


# ------------------------------------------------------------------ homogeneous
# The channel-to-lane maps.  A fresh engine hands out the slots of a group in
# the order its channels are opened (engine.hip open: local == nch++), and the
# kernels take slot c as
#   one lane per channel:  c = blockIdx.x * WG + threadIdx.x with WG a multiple of 64
#                          (demod_oqpsk_kernel's chain waves: pair = threadIdx.x & 255,
#                          demod_msk_kernel, demod_mskg_kernel, demod_c_kernel): wave c // 64
#                          (a generic-rate MSK group holds GENERIC_GROUP_CAP = 256 channels, a
#                          multiple of 64: channel j is slot j % 256 of group j // 256)
#   16 lanes per channel:  c = blockIdx.x * 4 + lane / 16 (demod_oqpskw_kernel,
#                          demod_mskw_kernel): wave c // 4
UNIT = {'one': 64, 'few': 4}


PART = 4  # classes per engine: 256 channels of a one-lane kernel, one generic-rate MSK group


def _homogeneous(ae, mode, shape, part):
    """The engine has no accessor for a channel's slot, so what is asserted here
    is only that the handles come in the order the channels were opened; that
    handle j is slot j, and slot c lane or lanes of wave c // copies, is read
    from the code (the comment above), not tested."""
    copies = UNIT[shape]
    kinds = ALL[part * PART:(part + 1) * PART]
    classes = [k for k in kinds for _ in range(copies)]
    chans = _compare(ae, mode, 'hop', True, classes, every_run=False, layout='homogeneous (%s)' % shape)
    assert chans == list(range(len(classes))), 'the handles are not the channels in their order'
    assert all(len(set(classes[w:w + copies])) == 1 for w in range(0, len(classes), copies))


PARTS = list(range(len(ALL) // PART))
assert len(PARTS) * PART == len(ALL)


@pytest.mark.parametrize('part', PARTS)
def test_homogeneous_oqpsk(engine_lib, oqpsk_kernel, part):
    import aero_engine as ae
    _homogeneous(ae, 'oqpsk10500@48000', oqpsk_kernel, part)


@pytest.mark.parametrize('part', PARTS)
def test_homogeneous_c(engine_lib, part):
    import aero_engine as ae
    _homogeneous(ae, 'c8400@48000', 'one', part)


@pytest.mark.parametrize('part', PARTS)
@pytest.mark.parametrize('mode', MSK_MODES)
def test_homogeneous_msk(engine_lib, msk_kernel, mode, part):
    import aero_engine as ae
    _homogeneous(ae, mode, msk_kernel, part)


# ------------------------------------------------------------------ beside silence
# the 16-lane kernels' waves of 4 channels: a silent class and three of the
# twelve classes that ORDER's waves of 4 never put beside one
BESIDE = (('silence', 'noise', 'tiny', 'negated'), ('one_sample', 'lead0', 'late', 'overlap'),
          ('lsb_noise', 'tone', 'tone_far', 'gated'), ('silence', 'cut_silence', 'cut_fullscale', 'cut_noise'))


@pytest.mark.parametrize('mode', ['oqpsk10500@48000'] + MSK_MODES)
def test_beside_silence_few(engine_lib, monkeypatch, mode):
    import aero_engine as ae
    monkeypatch.delenv('AERO_OQPSK_WIDE', raising=False)  # the 16-lane shapes (the default for so few channels)
    monkeypatch.delenv('AERO_MSK_WIDE', raising=False)
    waves4 = [xi.ORDER[w:w + 4] for w in range(0, len(xi.ORDER), 4)]
    lone = {n for w in waves4 if not set(w) & set(xi.SILENT) for n in w}
    assert len(lone) == 12 and lone == {n for w in BESIDE for n in w[1:]}
    assert all(w[0] in xi.SILENT for w in BESIDE)
    classes = [xi.ORDER.index(n) for w in BESIDE for n in w]
    chans = _compare(ae, mode, 'hop', True, classes, layout='beside silence (few)')
    assert chans == list(range(len(classes))), 'the handles are not the channels in their order'


# ------------------------------------------------------------------ two waves
@pytest.mark.parametrize('mode', ['oqpsk10500@48000', 'c8400@48000'])
def test_two_waves(engine_lib, monkeypatch, mode):
    """70 channels of a one-lane kernel: class k in lanes k, k + 20 and k + 40
    of the first wave; the partial second wave starts with two_samples, noise,
    tone, tiny, tone_far, negated"""
    import aero_engine as ae
    monkeypatch.setenv('AERO_OQPSK_WIDE', '0')
    n = len(xi.ORDER)
    classes = [j % n for j in range(64)] + [(j + 7) % n for j in range(6)]
    assert [xi.ORDER[k] for k in classes[64:]] == ['two_samples', 'noise', 'tone', 'tiny', 'tone_far', 'negated']
    assert all(classes[64 + j] != classes[j] for j in range(6))
    _compare(ae, mode, 'hop', True, classes, layout='two waves')
