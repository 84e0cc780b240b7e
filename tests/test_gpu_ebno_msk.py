"""AERO_F_EBNO_MSK on the GPU: the MSK Eb/N0 kernel (ebno.hip ebno_msk_kernel)
behind the MSK demod, bit for bit against the checker's estimator
(tools/oracle_ebno_msk.cpp, its own buffers), and aero_channel_get_quality /
aero_pop_ebno around it, for both MSK kernel shapes.

Streams, classes and cases: tests/ebno_msk_lib.py (4.4 Fs samples: past the
estimator's 2 Fs window and twice around the ring the kernel keeps).  The
checker's EbNo after sample k is series[k]; a channel that has demodulated n
samples holds series[n - 1], and a record of aero_pop_ebno with sample index n
(the hop record's field 0) carries that value."""
import numpy as np
import pytest

import aero_engine as ae
import aero_testlib as tl
import ebno_msk_lib as em

pytestmark = pytest.mark.gpu

TRACE = ae.F_TRACE_HOPS | ae.F_TRACE_SOFT | ae.F_TRACE_FRAMES
FLAG = getattr(ae, 'F_EBNO_MSK', 0)  # (0: an engine without the feature, whose MSK channels have no estimate)
NCH = 130  # three waves of the one-lane kernel, the last partial
CASE = '600@12000'


def _invalid(fn, *a):
    with pytest.raises(ae.AeroError) as ei:
        fn(*a)
    return ei.value.rc == ae.AERO_E_INVALID


def _bits1(v):
    return em.bits([v])[0]


class Follower:
    """one flagged channel against the checker's series: every record popped so far.  `fresh`: the
    sample counts at which the channel's estimator was constructed (0, and every rate change): a
    channel that stands there has taken nothing since and reports the model's start, 0.0"""

    def __init__(self, eng, ch, name, series, fresh=(0,)):
        self.eng, self.ch, self.name, self.series, self.fresh = eng, ch, name, series, set(fresh)
        self.eb = np.zeros((0, 2))
        self.hops = np.zeros((0, 6))

    def check(self, flushed=False):
        eng, ch = self.eng, self.ch
        self.eb = np.concatenate([self.eb, eng.ebno(ch)])
        self.hops = np.concatenate([self.hops, eng.hops(ch)])
        eb, hops = self.eb, self.hops
        idx = eb[:, 0].astype(np.int64)
        assert np.array_equal(idx.astype(np.float64), eb[:, 0]) and (idx >= 1).all(), self.name
        want = self.series[idx - 1]
        bad = np.flatnonzero(em.bits(eb[:, 1]) != em.bits(want))
        assert bad.size == 0, '%s: EbNo record of sample %d is %r, the checker has %r' % (
            self.name, idx[bad[0]], eb[bad[0], 1], want[bad[0]])
        # one record per hop record, with its sample index; a flush that ends on a boundary may leave one more
        assert len(hops) <= len(eb) <= len(hops) + (1 if flushed else 0), (self.name, len(hops), len(eb))
        assert np.array_equal(eb[:len(hops), 0], hops[:, 0]), self.name
        q = eng.channel_quality(ch)
        assert q['ebno_valid'] == 1
        if q['samples'] in self.fresh:
            assert q['ebno_db'] == 0.0, (self.name, q)
        else:
            assert _bits1(q['ebno_db']) == _bits1(self.series[q['samples'] - 1]), (self.name, q)
        if len(hops) and not flushed:
            # after a plain run the channel stands on its last hop's boundary
            last = hops[-1]
            got = [float(q['samples']), q['mse'], q['mixer_hz'], q['center_hz'], float(q['signal'])]
            assert np.array_equal(em.bits(got), em.bits(last[[0, 4, 2, 3, 5]])), (self.name, q, last)
            assert _bits1(q['ebno_db']) == _bits1(eb[len(hops) - 1, 1]), self.name
        return q


def _everything(eng, ch):
    return dict(soft=eng.softbits(ch), hops=eng.hops(ch), frames=eng.frames(ch), items=eng.items(ch))


def _stands(b):
    """where a channel stands after a plain run with b samples pushed"""
    return b // em.HOP * em.HOP - 1 if b >= em.HOP else 0


def test_classes_on_one_engine_and_flag_off(engine_lib, msk_kernel):
    n = em.n_of(CASE)
    names = [em.CLASSES[k % len(em.CLASSES)] for k in range(NCH)]
    pcm = np.stack([em.stream(CASE, k) for k in names], axis=1)
    with ae.Engine(NCH, flags=FLAG | TRACE) as on, ae.Engine(NCH, flags=TRACE) as off:
        for e in (on, off):
            assert [e.open_channel(600, 12000) for _ in range(NCH)] == list(range(NCH))
        fol = [Follower(on, c, names[c], em.reference(CASE, names[c])[0]) for c in range(NCH)]
        for a, b in em.messages(n, em.RAGGED):
            for e in (on, off):
                e.push_batch(pcm[a:b])
                e.run()
                e.sync()
            for f in fol:
                assert f.check()['samples'] == _stands(b)
        for e in (on, off):
            e.flush()
            e.sync()
        for f in fol:
            assert f.check(flushed=True)['samples'] == n
            assert len(f.eb) == n // em.HOP
            ref_hops = em.reference(CASE, f.name)[2]
            assert np.array_equal(em.bits(f.hops), em.bits(ref_hops)), f.name  # the oracle's, flag or no flag
        assert on.stat('ebno_launches') > 0 and off.stat('ebno_launches') == 0
        # the ring alone: 2 Fs doubles for each of the group's 192 slots
        assert on.stat('device_bytes') - off.stat('device_bytes') >= 16 * 12000 * 192
        for c in range(NCH):
            a, b = _everything(on, c), _everything(off, c)
            assert np.array_equal(a['soft'], b['soft']) and np.array_equal(a['frames'], b['frames']), names[c]
            assert a['items'] == b['items'], names[c]
            assert np.array_equal(em.bits(np.concatenate([fol[c].hops, a['hops']])), em.bits(b['hops'])), names[c]
            assert _invalid(off.ebno, c)
            q = off.channel_quality(c)
            assert q['ebno_valid'] == 0 and q['ebno_db'] == 0.0 and q['samples'] == n


@pytest.mark.parametrize('case', ['1200@24000', '600@18750'])
def test_other_rates(engine_lib, msk_kernel, case):
    """a compiled 24 kHz group and a generic-rate group (odd samples per symbol), two channels each"""
    bitrate, fs = em.CASES[case]
    n = em.n_of(case)
    names = ('synth10', 'one_sample')
    with ae.Engine(2, flags=FLAG | TRACE) as eng:
        chans = [eng.open_channel(bitrate, fs) for _ in names]
        fol = [Follower(eng, c, k, em.reference(case, k)[0]) for c, k in zip(chans, names)]
        for a, b in em.messages(n, em.RAGGED):
            for c, k in zip(chans, names):
                eng.push(c, em.stream(case, k)[a:b])
            eng.run()
            eng.sync()
            for f in fol:
                assert f.check()['samples'] == _stands(b)
        eng.flush()
        eng.sync()
        for f in fol:
            assert f.check(flushed=True)['samples'] == n
            assert len(f.eb) == n // em.HOP
            assert np.array_equal(em.bits(f.hops), em.bits(em.reference(case, f.name)[2])), f.name
        assert eng.stat('ebno_launches') > 0


def test_rate_change_starts_a_fresh_estimator(engine_lib, msk_kernel):
    """12 kHz, 24 kHz and 12 kHz again through push at changing rates: records and quality go on in the
    channel's own sample index, the estimate restarts with each move (the checker's is re-created)"""
    series, ref_hops = em.rate_reference()
    starts, p = [0], 0
    for k, _ in em.RATE_LEGS:
        p += k
        starts.append(p)
    with ae.Engine(2, flags=FLAG | TRACE) as eng:
        ch = eng.open_channel(600, em.RATE_LEGS[0][1])
        f = Follower(eng, ch, 'rate change', series, fresh=starts[:-1])
        base = 0
        for x, fs in em.rate_stream():
            for a, b in em.messages(len(x), em.RAGGED):
                eng.push(ch, x[a:b], fs)
                eng.run()
                eng.sync()
                # (a channel that has just moved was flushed at its old rate and stands off a boundary)
                q = f.check(flushed=True)
                assert q['samples'] == base + _stands(b)
            base += len(x)
        eng.flush()
        eng.sync()
        assert f.check(flushed=True)['samples'] == base == len(series)
        assert np.array_equal(em.bits(f.hops), em.bits(ref_hops))
        assert len(f.eb) == len(ref_hops) == sum(k // em.HOP for k, _ in em.RATE_LEGS)
        assert np.array_equal(f.eb[:, 0], ref_hops[:, 0])


def test_export_import_continues_the_series(engine_lib, msk_kernel):
    n, cut = em.n_of(CASE), 40000
    x, series = em.stream(CASE, 'synth10'), em.reference(CASE, 'synth10')[0]
    flags = FLAG | TRACE
    with ae.Engine(4, flags=flags) as src, ae.Engine(4, flags=flags) as dst, ae.Engine(4, flags=TRACE) as plain:
        ch = src.open_channel(600, 12000)
        f = Follower(src, ch, 'synth10', series)
        for a, b in em.messages(cut, (3000,)):
            src.push(ch, x[a:b])
            src.run()
            src.sync()
            f.check()
        blob = src.export_channel(ch)
        with pytest.raises(ae.AeroError) as ei:
            plain.import_channel(blob)
        assert ei.value.rc == ae.AERO_E_INVALID
        ch2 = dst.import_channel(blob)
        g = Follower(dst, ch2, 'synth10', series)
        assert g.check()['samples'] == _stands(cut)
        for a, b in em.messages(n - cut, (3000,)):
            dst.push(ch2, x[cut + a:cut + b])
            dst.run()
            dst.sync()
            g.check()
        dst.flush()
        dst.sync()
        assert g.check(flushed=True)['samples'] == n
        # the records go on where the source's stopped: together, every hop of the stream once
        assert np.array_equal(np.concatenate([f.eb[:, 0], g.eb[:, 0]]),
                              np.arange(1, n // em.HOP + 1) * float(em.HOP) - 1)


def test_close_and_reopen_starts_at_zero(engine_lib, msk_kernel):
    n1 = 26000  # past the 24000-sample window: the closed channel's ring is full
    s14, s10, s6 = (em.stream(CASE, 'synth%d' % k) for k in (14, 10, 6))
    with ae.Engine(2, flags=FLAG | TRACE) as eng:
        keep, ch = eng.open_channel(600, 12000), eng.open_channel(600, 12000)
        fk = Follower(eng, keep, 'synth14', em.reference(CASE, 'synth14')[0])
        for a, b in em.messages(n1, (3000,)):
            eng.push(keep, s14[a:b])
            eng.push(ch, s10[a:b])
            eng.run()
            eng.sync()
            fk.check()
        q = eng.channel_quality(ch)
        assert q['ebno_valid'] == 1 and q['ebno_db'] != 0.0
        eng.close_channel(ch)
        assert eng.open_channel(600, 12000) == ch
        q = eng.channel_quality(ch)
        assert q['samples'] == 0 and q['ebno_db'] == 0.0 and q['ebno_valid'] == 1
        # zero sums, ring and EbNo: the reopened channel follows a fresh channel's series
        f = Follower(eng, ch, 'synth6', em.reference(CASE, 'synth6')[0])
        for a, b in em.messages(n1, (3000,)):
            eng.push(keep, s14[n1 + a:n1 + b])
            eng.push(ch, s6[a:b])
            eng.run()
            eng.sync()
            fk.check()
            f.check()
        assert len(f.eb) == n1 // em.HOP and len(fk.eb) == 2 * n1 // em.HOP


def test_other_kinds_ignore_the_flag_and_f_ebno_alone_ignores_msk(engine_lib):
    msk = em.stream(CASE, 'synth10')[:12000]
    oq = tl.synth(seconds=0.5, seed=5, carrier=8000.0, ebn0=10.0)
    with ae.Engine(4, flags=FLAG | TRACE) as eng:
        o = eng.open_channel(10500)
        b = eng.open_channel(10500, burst=True)
        m = eng.open_channel(600, 12000)
        eng.push(o, oq[:12000])
        eng.push(m, msk)
        eng.run()
        eng.sync()
        q = eng.channel_quality(o)
        assert q['ebno_valid'] == 0 and q['ebno_db'] == 0.0 and q['samples'] == _stands_oqpsk(12000)
        assert _invalid(eng.ebno, o)
        assert _invalid(eng.channel_quality, b) and _invalid(eng.ebno, b)
        assert eng.channel_quality(m)['ebno_valid'] == 1 and len(eng.ebno(m)) == 12000 // em.HOP
        launches = eng.stat('ebno_launches')
        assert launches > 0
        eng.push(o, oq[12000:24000])
        eng.run()
        eng.sync()
        assert eng.stat('ebno_launches') == launches  # the OQPSK group launches none
    with ae.Engine(2, flags=ae.F_EBNO | TRACE) as eng:
        m = eng.open_channel(600, 12000)
        eng.push(m, msk)
        eng.run()
        eng.sync()
        q = eng.channel_quality(m)
        assert q['ebno_valid'] == 0 and q['ebno_db'] == 0.0 and q['samples'] == _stands(12000)
        assert _invalid(eng.ebno, m) and eng.stat('ebno_launches') == 0


def _stands_oqpsk(b):
    return b // 4096 * 4096 - 1 if b >= 4096 else 0


def test_without_hop_traces_passes_stay_asynchronous(engine_lib, msk_kernel):
    n = em.n_of(CASE)
    names = list(em.CLASSES)
    pcm = np.stack([em.stream(CASE, k) for k in names], axis=1)
    k = len(names)
    with ae.Engine(k, flags=FLAG) as fast, ae.Engine(k, flags=FLAG | TRACE) as traced:
        for e in (fast, traced):
            assert [e.open_channel(600, 12000) for _ in range(k)] == list(range(k))
        assert _invalid(fast.ebno, 0)  # no AERO_F_TRACE_HOPS: no records
        for a, b in em.messages(n, em.RAGGED):
            for e in (fast, traced):
                e.push_batch(pcm[a:b])
                e.run()
        for flush in (False, True):
            for e in (fast, traced):
                if flush:
                    e.flush()
                e.sync()
            for c in range(k):
                qa, qb = fast.channel_quality(c), traced.channel_quality(c)
                assert qa['samples'] == (n if flush else _stands(n))
                assert qa['ebno_valid'] == 1
                assert all(_bits1(qa[f]) == _bits1(qb[f]) for f in qa), (names[c], qa, qb)
                assert _bits1(qa['ebno_db']) == _bits1(em.reference(CASE, names[c])[0][qa['samples'] - 1])
        assert fast.stat('ebno_launches') > 0


def test_device_log10_on_the_arguments_this_estimator_adds(engine_lib):
    """negative, zero of either sign, subnormal and infinite arguments, which the OQPSK estimator's
    1e-9 floor never gave aero_log10: against glibc's log10 on the host (a NaN for a NaN)"""
    import mathhost
    x = np.array([-1.0, -0.0, 0.0, 5e-324, 2.2250738585072014e-308 / 3, 1e-310, np.inf, -np.inf, -1e-320, np.nan,
                  0.0085, 2.0])
    with ae.Engine(1) as eng:
        dev = eng.device_math('log10', x)
    host = mathhost.glibc('log10', x)
    nan = np.isnan(host)
    assert np.array_equal(np.isnan(dev), nan) and nan[0] and nan[7] and nan[8] and nan[9]
    assert np.array_equal(em.bits(dev[~nan]), em.bits(host[~nan])), (dev, host)
    assert np.isneginf(dev[1]) and np.isneginf(dev[2]) and np.isposinf(dev[6])
