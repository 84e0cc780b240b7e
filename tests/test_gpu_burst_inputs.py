"""The burst demodulators on adversarial PCM, bit for bit against the oracle.

Every class of tests/burst_inputs.py (silence, full scale, -32768, one sample,
1-LSB noise, a steady tone, noise, the gated carrier that stalls the front end
and the framing, gated carriers and noise whose checks are rejected, the
synthetic burst plain, clipped, at +-4 LSB, negated, from sample 0, behind an
AGC ring of zeros, cut off into silence, full scale and noise, and overlapping
itself) is a channel of one engine per kind, so a stalled lane, a silent lane
and a decoding lane share a wave.  tests/test_burst_inputs.py shows which
paths the classes reach.

Three message schedules (burst_inputs.runs: the largest message, two queued
per run(), sizes around the Hilbert block down to one sample), each with
AERO_F_DCD_TICK_BURST off and on; the oracle is fed the same messages (and
ticks).  burst_run (burst_engine.hip) repeats its pass until no channel has a
pushed sample undemodulated or a committed soft entry unframed, and the
Hilbert stage hands on every pushed sample (sample s needs the blocks below
s // 6145 only), so a run() delivers exactly what the oracle has delivered
after the same messages: after EVERY run() + sync() each channel's trident
records (f64 bit patterns), soft bits with their markers, R/T tests, R/T
packets and ACARS items so far EQUAL the oracle's so far, not merely a prefix
of its final ones; after flush() the DataCarrierDetect changes are equal too.

aero_stat "rt_pass_max" is the most R/T tests of one pass summed over the
group's channels, so on the engine with every class it can exceed
RT_TESTS_PER_PASS (asserted >=); on an engine with the stalling class alone
it is exactly that."""
import concurrent.futures as cf
import functools

import numpy as np
import pytest

import aero_testlib as tl  # noqa: F401  (puts the package on sys.path)
import burst_inputs as bi
import oracle_tick as ot

pytestmark = pytest.mark.gpu

TRACES = ('hops', 'soft', 'tests', 'packets', 'items')
RT_TESTS_PER_PASS = bi.RT_TESTS_PER_PASS  # burst_common.h; no Python binding


def _walk_class(kind, schedule, tick, pcm):
    """one oracle channel: (final outputs, per run() the length of every trace so far)"""
    o = bi.oracle(kind, tick)
    counts = []
    for grp in bi.runs(len(pcm), schedule):
        for a, b in grp:
            o.push(pcm[a:b])
        counts.append((len(o.hops()), len(o.softbits16()), len(o.rt_tests()), len(o.rt_packets()),
                       len(o.item_lines('A'))))
    final = ot.outputs(o)
    for v in final.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return final, tuple(counts)


@functools.lru_cache(maxsize=None)
def _reference(kind, schedule, tick):
    """The oracle per class at every checkpoint (its traces only grow: a
    checkpoint is a length of each final trace).  Computed once per kind,
    schedule and tick, shared by every engine layout, never changed."""
    bi.oracle(kind)  # the library is built and loaded before the threads start
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        futs = [ex.submit(_walk_class, kind, schedule, tick, pcm) for _, pcm in bi.streams(kind)]
        return tuple(f.result() for f in futs)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _first_diff(got, ref):
    """index of the first entry (row) of got that is not ref's, None if got == ref"""
    n = min(len(got), len(ref))
    if isinstance(ref, np.ndarray):
        width = int(np.prod(ref.shape[1:]))  # entries per row
        g, r = _bits(got[:n]).reshape(n, width), _bits(ref[:n]).reshape(n, width)
        bad = np.flatnonzero((g != r).any(axis=1))
    else:
        bad = [k for k in range(n) if got[k] != ref[k]]
    if len(bad):
        return int(bad[0])
    return None if len(got) == len(ref) else n


def _show(seq, k):
    return repr(seq[k]) if k < len(seq) else 'nothing (%d entries)' % len(seq)


def _take(eng, ch):
    return dict(hops=eng.hops(ch).reshape(-1, 6), soft=eng.softbits16(ch), tests=eng.rt_tests(ch).reshape(-1, 2),
                packets=eng.rt_packets(ch), items=eng.items(ch))


def _append(acc, new):
    for k in TRACES:
        acc[k] = acc[k] + new[k] if isinstance(new[k], list) else np.concatenate([acc[k], new[k]])


def _empty():
    return dict(hops=np.zeros((0, 6)), soft=np.zeros(0, np.int16), tests=np.zeros((0, 2), np.uint32), packets=[],
                items=[])


def _compare(ae, kind, schedule, tick, classes):
    """One engine whose channel j carries class classes[j]; every channel
    against the oracle after every run() and after flush().  Returns the
    engine's rt_pass_max."""
    names = [n for n, _ in bi.streams(kind)]
    pcms = [p for _, p in bi.streams(kind)]
    ref = _reference(kind, schedule, tick)
    bitrate = bi.KINDS[kind][0]
    plans = [bi.runs(len(pcms[k]), schedule) for k in classes]
    flags = ae.F_TRACE_SOFT | ae.F_TRACE_HOPS | ae.F_TRACE_FRAMES | (ae.F_DCD_TICK_BURST if tick else 0)
    eng = ae.Engine(max_channels=len(classes), flags=flags)
    try:
        chans = [eng.open_channel(bitrate, bi.FS, burst=True) for _ in classes]
        acc = [_empty() for _ in classes]

        def check(r, what):
            for j, k in enumerate(classes):
                final, counts = ref[k]
                _append(acc[j], _take(eng, chans[j]))
                want = counts[min(r, len(counts) - 1)]
                for t, n in zip(TRACES, want):
                    exp = final[t][:n]
                    bad = _first_diff(acc[j][t], exp)
                    assert bad is None, '%s %s%s, %s (channel %d), %s %d: %s differ at %d: %s (engine) %s (oracle)' % (
                        kind, schedule, ' ticked' if tick else '', names[k], j, what, r, t, bad,
                        _show(acc[j][t], bad), _show(exp, bad))

        for r in range(max(len(p) for p in plans)):
            depth = max(len(p[r]) for p in plans if r < len(p))
            for m in range(depth):  # the channels' queued messages interleaved
                for j, k in enumerate(classes):
                    if r < len(plans[j]) and m < len(plans[j][r]):
                        a, b = plans[j][r][m]
                        eng.push(chans[j], pcms[k][a:b])
            eng.run()
            eng.sync()
            check(r, 'after run')
        eng.flush()
        eng.sync()
        check(max(len(p) for p in plans), 'after flush, run')
        for j, k in enumerate(classes):
            got, want = eng.channel_events(chans[j])[0], ref[k][0]['edges']
            assert got == want, '%s %s%s, %s (channel %d): DataCarrierDetect changes %d (engine) %d (oracle)' % (
                kind, schedule, ' ticked' if tick else '', names[k], j, got, want)
        return eng.stat('rt_pass_max')
    finally:
        eng.close()


@pytest.mark.parametrize('tick', [False, True], ids=['untimed', 'ticked'])
@pytest.mark.parametrize('schedule', bi.SCHEDULES)
@pytest.mark.parametrize('kind', list(bi.KINDS))
def test_every_class_at_every_checkpoint(engine_lib, kind, schedule, tick):
    import aero_engine as ae
    pass_max = _compare(ae, kind, schedule, tick, list(range(len(bi.ORDER))))
    if kind == 'oqpsk10500':
        # the sum over the channels of a pass: a lane's own limit shows in test_stalling_class_alone
        assert pass_max >= RT_TESTS_PER_PASS, 'no pass reached the per-pass test limit (%d)' % pass_max


def test_stalling_class_alone(engine_lib):
    """one channel: no pass queues more than a lane's RT_TESTS_PER_PASS tests,
    and one does queue that many (the oracle runs 15 in one message)"""
    import aero_engine as ae
    pass_max = _compare(ae, 'oqpsk10500', 'max', False, [bi.ORDER.index('pulse_stall')])
    assert pass_max == RT_TESTS_PER_PASS


def test_two_waves(engine_lib):
    """70 channels: class k in lane k (and k + 20, k + 40, ...) of the first
    wave, the partial second wave starts with cut_fullscale, cut_noise,
    overlap, silence, pulse_stall, square (xcd_channel's map of 70
    workgroups, the last wave of the 64-lane kernels)"""
    import aero_engine as ae
    n = len(bi.ORDER)
    classes = [j % n for j in range(64)] + [(j + 17) % n for j in range(6)]
    assert [bi.ORDER[k] for k in classes[64:]] == ['cut_fullscale', 'cut_noise', 'overlap', 'silence', 'pulse_stall',
                                                   'square']
    assert all(classes[64 + j] != classes[j] for j in range(6))
    _compare(ae, 'oqpsk10500', 'max', True, classes)
