"""[vfos] entries that open, close, skip and change hands while the GPU
channeliser runs (aero_chan_vfo_open / _close / _skip / aero_chan_reserve,
include/aero_chan.h), against the always-present oracle
channeliser (oracle/pub_oracle.cpp).  Every comparison is bitwise on the int16
audio and the int8 IQ.  The model these tests rely on, a VFO started at read k
with zero histories equals an always-present one after `bound` samples and
from its first sample when the input was silent until then, is pinned on the
CPU by tests/test_chan_start_model.py.

max_blocks is 2 and reads are run in pairs, so histories cross read
boundaries inside a batch and between batches."""
import numpy as np
import pytest

import aero_testlib as tl
import chan_start_lib as cs

pytestmark = pytest.mark.gpu

CONFIGS = ['r1536k', 'r288k', 'r1920k']
CASES = [(name, v) for name in CONFIGS for v in range(len(tl.PUB_CONFIGS[name]['vfos']))]


def _chan(name, vfos=None, skip=None, host_out=True):
    import aero_engine as ae
    cfg = cs.config(name)
    return ae.Channeliser(cfg['sample_rate'], cs.C, cfg['mains'], cfg['vfos'] if vfos is None else vfos,
                          max_blocks=2, host_out=host_out, skip=skip)


def _push(chs, x, B, lo, hi, pending=0):
    """reads lo .. hi-1 of x to every channeliser, run in pairs; the last `pending` reads stay pushed, not run"""
    for b in range(lo, hi):
        for ch in chs:
            ch.push(x[b * B:(b + 1) * B])
            if (b - lo) % 2 == 1 and b < hi - pending:
                ch.run()
    if not pending:
        for ch in chs:
            ch.run()
            ch.sync()


def _same(want, got, what):
    assert len(want) == len(got), '%s: %d samples, expected %d' % (what, len(got), len(want))
    bad = np.flatnonzero(want != got)
    assert bad.size == 0, '%s: %d mismatches, first at %d (%d vs %d)' % (what, bad.size, bad[0], want[bad[0]],
                                                                         got[bad[0]])


def _invalid(fn, *a):
    import aero_engine as ae
    with pytest.raises(ae.AeroError) as e:
        fn(*a)
    assert e.value.rc == ae.AERO_E_INVALID


def _open_at(name, v, k, after, silent):
    """Creates without VFO v, takes k reads (the last one still pending), opens v, takes `after` more.
    Returns (ch, id map gpu -> oracle, oracle outputs, S of v)."""
    cfg = cs.config(name)
    n = k + after
    sil = (0, k) if silent else (0, 0)
    infos, usb, iq = cs.oracle(name, n, sil)
    x, B = cs.wideband(name, n, sil), cs.block_len(name)
    rest = [d for i, d in enumerate(cfg['vfos']) if i != v]
    ch = _chan(name, rest)
    _push([ch], x, B, 0, k, pending=1)
    vid = ch.open_vfo(cfg['vfos'][v])
    assert vid == len(rest) == ch.vfo_count() - 1, 'the smallest free id'
    _push([ch], x, B, k, n)
    ids = {i: (i if i < v else i + 1) for i in range(len(rest))}
    ids[vid] = v
    return ch, ids, (infos, usb, iq), vid


def _others_exact(ch, ids, vid, usb, iq):
    for g, o in ids.items():
        if g != vid:
            _same(usb[o], ch.audio(g), 'vfo %d' % o)
    for m in range(len(iq)):
        _same(iq[m], ch.iq(m), 'main %d IQ' % m)


@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('name,v', CASES)
def test_open_under_live_input(name, v, k):
    cfg = cs.config(name)
    after = cfg['sample_rate'] // cs.block_len(name) + 2  # bufsplit + 2: the whole NCO table is walked
    ch, ids, (infos, usb, iq), vid = _open_at(name, v, k, after, silent=False)
    S, settle, b = infos[v]['samples_per_block'], ch.settle(vid), cs.bound(cfg, infos[v])
    assert ch.vfo_info(vid)['samples_per_block'] == S
    got = ch.audio(vid)
    assert len(got) == after * S
    assert settle <= b < S
    bad = np.flatnonzero(usb[v][k * S:] != got)
    print('%s vfo %d k %d: last differing sample %d, settle %d, bound %d' % (
        name, v, k, bad.max() if bad.size else -1, settle, b))
    _same(usb[v][k * S + settle:], got[settle:], 'opened vfo %d after its settle' % v)
    assert np.count_nonzero(got[settle:]) > (len(got) - settle) // 2
    _others_exact(ch, ids, vid, usb, iq)
    ch.close()


@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('name,v', CASES)
def test_silent_lead_in_exact_from_first_sample(name, v, k):
    ch, ids, (infos, usb, iq), vid = _open_at(name, v, k, 2, silent=True)
    S = infos[v]['samples_per_block']
    assert np.count_nonzero(usb[v][k * S:]) > S
    _same(usb[v][k * S:], ch.audio(vid), 'opened vfo %d' % v)
    _others_exact(ch, ids, vid, usb, iq)
    ch.close()


# closing both VFOs of r1536k's second main VFO stops that main VFO: it must
# come back with zero half-band history as well
@pytest.mark.parametrize('name,vs', [('r288k', [1]), ('r1920k', [2]), ('r1536k', [2, 3])])
def test_close_and_slot_reuse(name, vs):
    cfg = cs.config(name)
    k, n = 3, 6
    sil = (k, k + 1)
    infos, usb, iq = cs.oracle(name, n, sil)
    x, B = cs.wideband(name, n, sil), cs.block_len(name)
    nv = len(cfg['vfos'])
    ch = _chan(name)
    _push([ch], x, B, 0, k, pending=1)
    head = {}
    for v in vs:
        # the close runs the pending read with v; its audio has to be popped before
        ch.run()
        ch.sync()
        head[v] = ch.audio(v)
        ch.close_vfo(v)
    assert ch.stat('slots_free') == len(vs)
    for v in vs:
        S = infos[v]['samples_per_block']
        _same(usb[v][:k * S], head[v], 'vfo %d before its close' % v)
        for call in (ch.vfo_info, ch.audio, ch.output_device, ch.settle, ch.close_vfo):
            _invalid(call, v)
        _invalid(ch.skip_vfo, v, True)
        _invalid(ch.skip_vfo, v, False)
    assert ch.vfo_count() == (nv if max(vs) < nv - 1 else min(vs))
    nbytes = ch.stat('device_bytes')
    _push([ch], x, B, k, k + 1)  # one read of zeros
    for i, v in enumerate(vs):
        assert ch.stat('slots_free') == len(vs) - i
        assert ch.open_vfo(cfg['vfos'][v]) == v, 'the same id comes back'
    assert ch.stat('slots_free') == 0
    assert ch.stat('device_bytes') == nbytes
    assert ch.vfo_count() == nv
    _push([ch], x, B, k + 1, n)
    assert ch.stat('device_bytes') == nbytes
    for v in range(nv):
        S = infos[v]['samples_per_block']
        if v in vs:
            first = usb[v][(k + 1) * S:(k + 1) * S + cs.bound(cfg, infos[v])]
            assert np.count_nonzero(first) > 0, 'the samples that a stale history would change carry signal'
            _same(usb[v][(k + 1) * S:], ch.audio(v), 'reopened vfo %d from its first sample' % v)
        else:
            _same(usb[v], ch.audio(v), 'vfo %d' % v)
    for m in range(len(iq)):
        _same(iq[m], ch.iq(m), 'main %d IQ' % m)
    ch.close()


@pytest.mark.parametrize('name,v,k', [('r1920k', 2, 2), ('r288k', 1, 1), ('r1536k', 3, 3)])
def test_hand_over_on_one_card(name, v, k):
    cfg = cs.config(name)
    n = k + 2
    infos, usb, _ = cs.oracle(name, n)
    x, B = cs.wideband(name, n), cs.block_len(name)
    nv, S = len(cfg['vfos']), infos[v]['samples_per_block']
    a = _chan(name)
    b = _chan(name, skip=[i == v for i in range(nv)])
    assert b.vfo_count() == nv and b.vfo_info(v)['samples_per_block'] == S
    _push([a, b], x, B, 0, k - 1)
    b.skip_vfo(v, False)  # one read before the owner lets go
    _push([a, b], x, B, k - 1, k)
    a.skip_vfo(v, True)
    assert a.stat('slots_free') == 1 and b.stat('slots_free') == 0
    _push([a, b], x, B, k, n)
    assert b.settle(v) < S
    got_a, got_b = a.audio(v), b.audio(v)
    assert len(got_a) == k * S and len(got_b) == (n - k + 1) * S
    _same(usb[v], np.concatenate([got_a, got_b[S:]]), 'vfo %d across the hand-over' % v)
    for o in range(nv):
        if o != v:
            _same(usb[o], a.audio(o), 'A vfo %d' % o)
            _same(usb[o], b.audio(o), 'B vfo %d' % o)
    a.close()
    b.close()


@pytest.mark.parametrize('reserve', [False, True])
def test_batch_of_opens_one_start(reserve):
    cfg = cs.config('c5')
    k, n, first = 1, 3, 48
    infos, usb, _ = cs.oracle('c5', n)
    x, B = cs.wideband('c5', n), cs.block_len('c5')
    late = cfg['vfos'][first:]
    assert len(cfg['vfos']) == 64
    ch = _chan('c5', cfg['vfos'][:first])
    if reserve:
        shapes = {}
        for d in late:
            shapes.setdefault((d['data_rate'], d.get('filter_bandwidth', 0)), []).append(d)
        for ds in shapes.values():
            ch.reserve(ds[0], len(ds))
        assert ch.stat('slots_free') == len(late)
    _push([ch], x, B, 0, k)
    inits, nbytes = ch.stat('vfo_inits'), ch.stat('device_bytes')
    for i, d in enumerate(late):
        assert ch.open_vfo(d) == first + i
    assert ch.stat('vfo_inits') == inits, 'the start waits for the next read'
    _push([ch], x, B, k, n)
    assert ch.stat('vfo_inits') == inits + 1, 'one start kernel for the batch'
    if reserve:
        assert ch.stat('device_bytes') == nbytes and ch.stat('slots_free') == 0
    else:
        assert ch.stat('device_bytes') > nbytes
    for v in range(64):
        S = infos[v]['samples_per_block']
        if v < first:
            _same(usb[v], ch.audio(v), 'vfo %d' % v)
        else:
            settle = ch.settle(v)
            assert settle <= cs.bound(cfg, infos[v]) < S
            _same(usb[v][k * S + settle:], ch.audio(v)[settle:], 'opened vfo %d after its settle' % v)
    ch.close()


def test_opened_vfo_into_the_decoder():
    """Silent lead-in, then the opened VFO's audio goes into an engine channel
    opened at the same moment: hops and soft bits of the oracle decoder on the
    oracle channeliser's audio."""
    import aero_engine as ae
    name, v, k, n = 'r288k', 0, 1, 11
    cfg = cs.config(name)
    sil = (0, k)
    infos, usb, _ = cs.oracle(name, n, sil)
    x, B = cs.wideband(name, n, sil), cs.block_len(name)
    S = infos[v]['samples_per_block']
    rest = [d for i, d in enumerate(cfg['vfos']) if i != v]
    ch = _chan(name, rest, host_out=False)
    eng = ae.Engine(max_channels=4, flags=ae.F_TRACE_HOPS | ae.F_TRACE_SOFT)
    chans = [-1] * len(rest)
    for b in range(n):
        if b == k:
            vid = ch.open_vfo(cfg['vfos'][v])
            chans = [-1] * ch.vfo_count()
            chans[vid] = eng.open_channel(ae.vfo_bitrate(cfg['vfos'][v]['data_rate']))
        ch.push(x[b * B:(b + 1) * B])
        ch.run()
        ch.feed(eng, chans)
        eng.run()
    eng.flush()
    o = tl.Oracle(bitrate=ae.vfo_bitrate(cfg['vfos'][v]['data_rate']))
    o.push_chunked(usb[v][k * S:], S)
    h, rh = eng.hops(chans[vid]), o.hops()
    assert len(h) == len(rh) > 0
    assert np.array_equal(h.view(np.int64), rh.view(np.int64))
    assert np.array_equal(eng.softbits(chans[vid]), o.softbits())
    eng.close()
    ch.close()


def test_errors():
    cfg = cs.config('r1536k')
    ch = _chan('r1536k')
    nv = len(cfg['vfos'])
    far = dict(cfg['vfos'][0], frequency=cs.C + 350000)  # between the second and third main VFO
    _invalid(ch.open_vfo, far)
    _invalid(ch.open_vfo, dict(cfg['vfos'][0], frequency=cs.C + 610000))  # under the IQ-publishing main VFO
    _invalid(ch.open_vfo, dict(cfg['vfos'][0], data_rate=0, out_rate=0))
    _invalid(ch.reserve, cfg['vfos'][0], 0)
    _invalid(ch.reserve, cfg['vfos'][0], -1)
    _invalid(ch.reserve, far, 1)
    _invalid(ch.stat, 'no_such_counter')
    assert ch.vfo_count() == nv and ch.stat('slots_free') == 0
    ch.close_vfo(1)
    _invalid(ch.close_vfo, 1)
    _invalid(ch.skip_vfo, 1, True)
    _invalid(ch.skip_vfo, 1, False)
    _invalid(ch.close_vfo, nv)
    _invalid(ch.close_vfo, -1)
    assert ch.vfo_count() == nv
    ch.close_vfo(nv - 1)
    assert ch.vfo_count() == nv - 1
    ch.skip_vfo(0, True)
    ch.skip_vfo(0, True)  # already skipped: nothing to do
    assert ch.stat('slots_free') == 3
    ch.skip_vfo(0, False)
    assert ch.stat('slots_free') == 2
    assert ch.open_vfo(cfg['vfos'][1]) == 1 and ch.open_vfo(cfg['vfos'][3]) == nv - 1
    assert ch.stat('slots_free') == 0 and ch.vfo_count() == nv
    ch.close()
