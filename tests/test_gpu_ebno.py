"""AERO_F_EBNO on the GPU: the Eb/N0 kernel (ebno.hip) behind the demod, bit for
bit against the checker's estimator (tools/oracle_ebno.cpp, its own buffers),
and aero_channel_get_quality / aero_pop_ebno around it.

Streams and classes: tests/ebno_lib.py (201600 samples: past the estimator's
window and past one wrap of the AGC ring the kernel reads).  The checker's
EbNo after sample k is series[k]; a channel that has demodulated n samples
holds series[n - 1], and a record of aero_pop_ebno with sample index n (the
hop record's field 0) carries that value."""
import numpy as np
import pytest

import aero_engine as ae
import aero_testlib as tl
import ebno_lib as el

pytestmark = pytest.mark.gpu

TRACE = ae.F_TRACE_HOPS | ae.F_TRACE_SOFT | ae.F_TRACE_FRAMES
NCH = 130  # three waves of the one-lane kernel, the last partial


def _invalid(fn, *a):
    with pytest.raises(ae.AeroError) as ei:
        fn(*a)
    return ei.value.rc == ae.AERO_E_INVALID


class Follower:
    """one flagged channel against the checker's series: every record popped so far"""

    def __init__(self, eng, ch, name, series=None):
        self.eng, self.ch, self.name = eng, ch, name
        self.series = el.reference(name)[0] if series is None else series
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
        bad = np.flatnonzero(el.bits(eb[:, 1]) != el.bits(want))
        assert bad.size == 0, '%s: EbNo record of sample %d is %r, the checker has %r' % (
            self.name, idx[bad[0]], eb[bad[0], 1], want[bad[0]])
        # one record per hop record, with its sample index; a flush that ends on a boundary may leave one more
        assert len(hops) <= len(eb) <= len(hops) + (1 if flushed else 0), (self.name, len(hops), len(eb))
        assert np.array_equal(eb[:len(hops), 0], hops[:, 0]), self.name
        q = eng.channel_quality(ch)
        assert q['ebno_valid'] == 1
        if q['samples'] > 0:
            assert el.bits([q['ebno_db']])[0] == el.bits([self.series[q['samples'] - 1]])[0], (self.name, q)
        else:
            assert q['ebno_db'] == 0.0
        if len(hops) and not flushed:
            # after a plain run the channel stands on its last hop's boundary
            last = hops[-1]
            got = [float(q['samples']), q['mse'], q['mixer_hz'], q['center_hz'], float(q['signal'])]
            assert np.array_equal(el.bits(got), el.bits(last[[0, 4, 2, 3, 5]])), (self.name, q, last)
            assert el.bits([q['ebno_db']])[0] == el.bits([eb[len(hops) - 1, 1]])[0], self.name
        return q


def _everything(eng, ch):
    return dict(soft=eng.softbits(ch), hops=eng.hops(ch), frames=eng.frames(ch), items=eng.items(ch))


def test_classes_on_one_engine_and_flag_off(engine_lib, oqpsk_kernel):
    names = [el.OQPSK[k % len(el.OQPSK)] for k in range(NCH)]
    pcm = np.stack([el.stream(n) for n in names], axis=1)
    with ae.Engine(NCH, flags=ae.F_EBNO | TRACE) as on, ae.Engine(NCH, flags=TRACE) as off:
        for e in (on, off):
            assert [e.open_channel(10500) for _ in range(NCH)] == list(range(NCH))
        fol = [Follower(on, c, names[c]) for c in range(NCH)]
        for a, b in el.messages(el.N, el.RAGGED):
            for e in (on, off):
                e.push_batch(pcm[a:b])
                e.run()
                e.sync()
            for f in fol:
                q = f.check()
                assert q['samples'] == (b // el.HOP * el.HOP - 1 if b >= el.HOP else 0)
        for e in (on, off):
            e.flush()
            e.sync()
        for f in fol:
            assert f.check(flushed=True)['samples'] == el.N
            assert len(f.eb) == el.N // el.HOP
            ref_hops = el.reference(f.name)[2]
            assert np.array_equal(el.bits(f.hops), el.bits(ref_hops)), f.name  # the oracle's, flag or no flag
        assert on.stat('ebno_launches') > 0 and off.stat('ebno_launches') == 0
        assert on.stat('device_bytes') > off.stat('device_bytes')
        for c in range(NCH):
            a, b = _everything(on, c), _everything(off, c)
            assert np.array_equal(a['soft'], b['soft']) and np.array_equal(a['frames'], b['frames']), names[c]
            assert a['items'] == b['items'], names[c]
            assert np.array_equal(el.bits(np.concatenate([fol[c].hops, a['hops']])),
                                  el.bits(b['hops'])), names[c]
            assert _invalid(off.ebno, c)
            q = off.channel_quality(c)
            assert q['ebno_valid'] == 0 and q['ebno_db'] == 0.0 and q['samples'] == el.N
        assert sum(len(on.items(c)) for c in range(NCH)) == 0  # (popped above)


def test_c_channel_in_messages(engine_lib):
    series = el.reference('c', (el.C_MESSAGE,))[0]
    x = el.stream('c')
    with ae.Engine(2, flags=ae.F_EBNO | TRACE) as eng:
        chans = [eng.open_channel(8400), eng.open_channel(8400)]
        fol = [Follower(eng, c, 'c', series) for c in chans]
        for a, b in el.messages(el.N, (el.C_MESSAGE,)):
            for c in chans:
                eng.push(c, x[a:b])
            eng.run()
            eng.sync()
            for f in fol:
                # samples may stand on a message end: Follower checks ebno_db == series[samples - 1]
                f.check(flushed=True)
        eng.flush()
        eng.sync()
        for f in fol:
            assert f.check(flushed=True)['samples'] == el.N
            assert len(f.eb) == el.N // el.HOP
        assert eng.stat('ebno_launches') > 0


def test_export_import_continues_the_series(engine_lib, oqpsk_kernel):
    x, cut = el.stream('synth10'), 110000
    flags = ae.F_EBNO | TRACE
    with ae.Engine(4, flags=flags) as src, ae.Engine(4, flags=flags) as dst, ae.Engine(4, flags=TRACE) as plain:
        ch = src.open_channel(10500)
        f = Follower(src, ch, 'synth10')
        for a, b in el.messages(cut, (12000,)):
            src.push(ch, x[a:b])
            src.run()
            src.sync()
            f.check()
        blob = src.export_channel(ch)
        with pytest.raises(ae.AeroError) as ei:
            plain.import_channel(blob)
        assert ei.value.rc == ae.AERO_E_INVALID
        ch2 = dst.import_channel(blob)
        g = Follower(dst, ch2, 'synth10')
        assert g.check()['samples'] == cut // el.HOP * el.HOP - 1
        for a, b in el.messages(el.N - cut, (12000,)):
            dst.push(ch2, x[cut + a:cut + b])
            dst.run()
            dst.sync()
            g.check()
        dst.flush()
        dst.sync()
        assert g.check(flushed=True)['samples'] == el.N
        # the records go on where the source's stopped: together, every hop of the stream once
        assert np.array_equal(np.concatenate([f.eb[:, 0], g.eb[:, 0]]),
                              np.arange(1, el.N // el.HOP + 1) * float(el.HOP) - 1)


def test_close_and_reopen_starts_at_zero(engine_lib, oqpsk_kernel):
    with ae.Engine(2, flags=ae.F_EBNO | TRACE) as eng:
        keep, ch = eng.open_channel(10500), eng.open_channel(10500)
        fk = Follower(eng, keep, 'synth14')
        n1 = 60000
        for a, b in el.messages(n1, (12000,)):
            eng.push(keep, el.stream('synth14')[a:b])
            eng.push(ch, el.stream('synth10')[a:b])
            eng.run()
            eng.sync()
            fk.check()
        assert eng.channel_quality(ch)['ebno_db'] > 0.0
        eng.close_channel(ch)
        assert eng.open_channel(10500) == ch
        q = eng.channel_quality(ch)
        assert q['samples'] == 0 and q['ebno_db'] == 0.0 and q['ebno_valid'] == 1
        # zero sums and EbNo 0: the reopened channel follows a fresh channel's series
        f = Follower(eng, ch, 'synth6')
        for a, b in el.messages(n1, (12000,)):
            eng.push(keep, el.stream('synth14')[n1 + a:n1 + b])
            eng.push(ch, el.stream('synth6')[a:b])
            eng.run()
            eng.sync()
            fk.check()
            f.check()
        assert len(f.eb) == n1 // el.HOP and len(fk.eb) == 2 * n1 // el.HOP


def test_msk_and_burst_have_no_estimate(engine_lib):
    pcm = tl.synth_msk(seconds=4.0, bitrate=600, carrier=600.0)
    with ae.Engine(4, flags=ae.F_EBNO | TRACE) as eng:
        m = eng.open_channel(600)
        b = eng.open_channel(10500, burst=True)
        hops = np.zeros((0, 6))
        for i in range(0, len(pcm), 6000):
            eng.push(m, pcm[i:i + 6000])
            eng.run()
            eng.sync()
            hops = np.concatenate([hops, eng.hops(m)])
            q = eng.channel_quality(m)
            assert q['ebno_valid'] == 0 and q['ebno_db'] == 0.0
            if len(hops):
                got = [float(q['samples']), q['mse'], q['mixer_hz'], q['center_hz'], float(q['signal'])]
                assert np.array_equal(el.bits(got), el.bits(hops[-1][[0, 4, 2, 3, 5]])), (q, hops[-1])
        assert len(hops) == len(pcm) // 2048 and set(hops[:, 5]) <= {0.0, 1.0}
        assert _invalid(eng.ebno, m)
        assert _invalid(eng.channel_quality, b) and _invalid(eng.ebno, b)
        assert _invalid(eng.channel_quality, 3) and _invalid(eng.ebno, 3)  # never opened
        assert eng.stat('ebno_launches') == 0


def test_without_hop_traces_passes_stay_asynchronous(engine_lib, oqpsk_kernel):
    names = list(el.OQPSK)
    pcm = np.stack([el.stream(n) for n in names], axis=1)
    k = len(names)
    with ae.Engine(k, flags=ae.F_EBNO) as fast, ae.Engine(k, flags=ae.F_EBNO | TRACE) as traced:
        for e in (fast, traced):
            assert [e.open_channel(10500) for _ in range(k)] == list(range(k))
        assert _invalid(fast.ebno, 0)  # no AERO_F_TRACE_HOPS: no records
        for a, b in el.messages(el.N, el.RAGGED):
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
                assert qa['samples'] == (el.N if flush else el.N // el.HOP * el.HOP - 1)
                assert qa['ebno_valid'] == 1
                assert all(el.bits([qa[f]])[0] == el.bits([qb[f]])[0] for f in qa), (names[c], qa, qb)
                assert el.bits([qa['ebno_db']])[0] == el.bits([el.reference(names[c])[0][qa['samples'] - 1]])[0]
        assert fast.stat('ebno_launches') > 0
