"""aero_channel_close / aero_engine_reserve on the GPU.

A closed channel's id and slot go to the next open, and the reopened channel
is indistinguishable from the first channel of a new engine: everything it
emits equals a fresh oracle on its own stream (hop indices, DCD edges and
event counters from its first sample), while its neighbours equal oracles run
over their uninterrupted streams, bit for bit, for every channel kind.  The
slot's device state comes from the reset kernel (csrc/slot_reset.hip), so a
per-channel array it missed shows here as a reopened channel that differs
from its oracle.  Then the closed id's error returns, the id and slot order,
group sizing by reserve, churn in a reserved pool and the release of a
generic-rate group by its last close."""
import concurrent.futures as cf
import ctypes

import numpy as np
import pytest

import aero_testlib as tl

pytestmark = pytest.mark.gpu

SEC_A = 6.0  # before the close: the 4-s AGC ring full, the loops locked, a message in flight
C_SIZES = [4800, 2047, 12000, 2049, 9600, 100, 6143, 2048]  # ragged C-channel messages


def _kinds():
    import aero_engine as ae
    p = ae.F_TRACE_SOFT | ae.F_TRACE_HOPS | ae.F_TRACE_FRAMES
    return {
        # open_channel arguments, engine flags, message sizes, seconds of the replacement stream, seed of the
        # kind's streams (chosen so that each reference holds a frame or a packet), stream generator (seed,
        # seconds, channel), oracle
        'oqpsk': dict(open=dict(bitrate=10500), flags=p | ae.F_DCD_TICK, sizes=[12000], sec_d=6.0,
                      seed=0xC105E0 + 16, fs=None,
                      synth=lambda seed, sec, k: tl.synth(seconds=sec, seed=seed, carrier=12037.5 - 900.0 * k,
                                                          ebn0=12.0),
                      oracle=lambda: tl.Oracle(dcd_tick=True)),
        'msk600': dict(open=dict(bitrate=600), flags=p, sizes=[3000], sec_d=8.0, seed=0xC105E0 + 32, fs=12000,
                       synth=lambda seed, sec, k: tl.synth_msk(seconds=sec, bitrate=600, seed=seed,
                                                               carrier=600.0 + 400.0 * (k % 3), ebn0=14.0),
                       oracle=lambda: tl.Oracle(bitrate=600)),
        'msk1200': dict(open=dict(bitrate=1200), flags=p, sizes=[6000], sec_d=8.0, seed=0xC10640, fs=24000,
                        synth=lambda seed, sec, k: tl.synth_msk(seconds=sec, bitrate=1200, baud=600, seed=seed,
                                                                carrier=600.0 + 10.0 * (k % 3), ebn0=14.0),
                        oracle=lambda: tl.Oracle(bitrate=1200)),
        'msk600_16000': dict(open=dict(bitrate=600, fs=16000), flags=p, sizes=[4000], sec_d=8.0,
                             seed=0xC105E0 + 64, fs=16000,
                             synth=lambda seed, sec, k: tl.synth_msk(seconds=sec, bitrate=600, seed=seed,
                                                                     carrier=600.0 + 400.0 * (k % 3), ebn0=14.0,
                                                                     fs=16000),
                             oracle=lambda: tl.Oracle(bitrate=600)),
        'c8400': dict(open=dict(bitrate=8400), flags=p | ae.F_TRACE_PT, sizes=C_SIZES, sec_d=6.0,
                      seed=0xC105E0 + 80, fs=None,
                      synth=lambda seed, sec, k: tl.synth_c(seconds=sec, seed=seed, carrier=12000.0 - 1500.0 * k,
                                                            ebn0=12.0),
                      oracle=lambda: tl.Oracle(bitrate=8400, trace_pt=True)),
        'burst_oqpsk': dict(open=dict(bitrate=10500, burst=True), flags=p, sizes=[12000], sec_d=8.0,
                            seed=0xC105E0 + 96, fs=None,
                            synth=lambda seed, sec, k: tl.synth_burst(seconds=sec, seed=seed,
                                                                      carrier=12000.0 + 300.0 * k, ebn0=14.0),
                            oracle=lambda: tl.Oracle(burst=True)),
        'burst_msk1200': dict(open=dict(bitrate=1200, fs=48000, burst=True), flags=p, sizes=[12000], sec_d=8.0,
                              seed=0xC105E0 + 112, fs=None,
                              synth=lambda seed, sec, k: tl.synth_burst_msk(seconds=sec, bitrate=1200, seed=seed,
                                                                            carrier=2500.0 + 400.0 * k, ebn0=14.0),
                              oracle=lambda: tl.Oracle(bitrate=1200, burst=True)),
    }


def _messages(x, sizes, k0=0):
    out, p, k = [], 0, k0
    while p < len(x):
        n = sizes[k % len(sizes)]
        out.append(x[p:p + n])
        p += n
        k += 1
    return out


def _reference(kind, msgs, K=None):
    """everything a fresh oracle emits for these messages"""
    K = K or _kinds()[kind]
    o = K['oracle']()
    for m in msgs:
        o.push(m, fs=K['fs'])
    burst = 'burst' in kind
    r = dict(hops=o.hops(), items=o.item_lines('A'), events=o.events())
    if burst:
        r.update(soft=o.softbits16(), tests=o.rt_tests(), packets=o.rt_packets())
    else:
        r.update(soft=o.softbits(), frames=o.frames())
    if kind == 'c8400':
        r.update(pt=o.pt(), c_units=o.c_units(), voice=o.voice())
    return r


def _compare(eng, ch, kind, r, what):
    burst = 'burst' in kind
    sb = eng.softbits16(ch) if burst else eng.softbits(ch)
    assert len(sb) == len(r['soft']) and np.array_equal(sb, r['soft']), '%s: soft bits differ' % what
    h = eng.hops(ch)
    assert h.shape == r['hops'].shape and np.array_equal(h.view(np.int64), r['hops'].view(np.int64)), \
        '%s: hop records differ' % what
    dcd, steps, fcs = eng.channel_events(ch)
    if burst:
        assert np.array_equal(eng.rt_tests(ch), r['tests']), '%s: R/T tests differ' % what
        assert eng.rt_packets(ch) == r['packets'], '%s: R/T packets differ' % what
        assert (dcd, steps) == (r['events'][0], 0), '%s: DCD changes differ' % what
    else:
        assert np.array_equal(eng.frames(ch), r['frames']), '%s: frames differ' % what
        assert dcd == r['events'][0], '%s: DCD changes differ' % what
    if kind == 'c8400':
        pt = eng.pt(ch)
        assert pt.shape == r['pt'].shape and np.array_equal(pt.view(np.int64), r['pt'].view(np.int64)), \
            '%s: pt differs' % what
        assert np.array_equal(eng.c_units(ch), r['c_units']), '%s: Call_progress SUs differ' % what
        assert eng.voice(ch) == r['voice'], '%s: voice frames differ' % what
    else:
        assert eng.items(ch) == r['items'], '%s: items differ' % what
        if not burst:
            assert steps == len(r['events'][1]) and fcs == r['events'][1][-8:], '%s: hunter steps differ' % what


def _produced(kind, r):
    """the reference is not an empty comparison"""
    n = len(r['packets']) if 'burst' in kind else len(r['frames']) // 320
    return len(r['soft']) > 1000 and n >= 1


def _set_shape(monkeypatch, kind, shape):
    var = 'AERO_OQPSK_WIDE' if kind == 'oqpsk' else 'AERO_MSK_WIDE'
    if shape == 'one':
        monkeypatch.setenv(var, '0')
    else:
        monkeypatch.delenv(var, raising=False)


@pytest.fixture(scope='module')
def reuse_refs(cpu_libs):
    """per kind: the three channels' messages (A0, A1, A2), the replacement
    stream's (D), and the oracles of A0, A2 and D; computed once"""
    out = {}
    jobs = {}
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        for kind, K in sorted(_kinds().items()):
            total = SEC_A + K['sec_d']
            a = [_messages(K['synth'](K['seed'] + k, SEC_A if k == 1 else total, k), K['sizes'], k) for k in range(3)]
            d = _messages(K['synth'](K['seed'] + 3, K['sec_d'], 3), K['sizes'], 5)
            out[kind] = dict(a=a, d=d)
            jobs[kind] = [ex.submit(_reference, kind, m) for m in (a[0], a[2], d)]
        for kind, js in jobs.items():
            out[kind]['refs'] = [j.result() for j in js]
    return out


@pytest.mark.parametrize('kind,shape', [('oqpsk', 'few'), ('oqpsk', 'one'), ('msk600', 'few'), ('msk600', 'one'),
                                        ('msk1200', 'few'), ('msk600_16000', 'few'), ('c8400', 'few'),
                                        ('burst_oqpsk', 'few'), ('burst_msk1200', 'few')])
def test_reuse_equals_fresh_neighbours_undisturbed(engine_lib, reuse_refs, monkeypatch, kind, shape):
    import aero_engine as ae
    _set_shape(monkeypatch, kind, shape)
    K = _kinds()[kind]
    a, d = reuse_refs[kind]['a'], reuse_refs[kind]['d']
    r0, r2, rd = reuse_refs[kind]['refs']
    assert _produced(kind, rd) and _produced(kind, r0) and _produced(kind, r2), 'the oracle produced too little'
    eng = ae.Engine(max_channels=3, flags=K['flags'])
    chans = [eng.open_channel(**K['open']) for _ in range(3)]
    assert chans == [0, 1, 2]
    rounds = len(a[1])  # the messages of the 6 s before the close
    for r in range(rounds):
        for k in range(3):
            eng.push(chans[k], a[k][r])
        eng.run()
    if kind == 'c8400':
        eng.push(1, a[0][0])  # pushed after the last run: queued, not prefiltered, at the close
    eng.close_channel(1)  # straight after the run: no sync, nothing popped
    assert eng.open_channel(**K['open']) == 1
    r = rounds
    while r < max(len(a[0]), len(a[2]), rounds + len(d)):
        for ch, m in ((0, a[0]), (2, a[2])):
            if r < len(m):
                eng.push(ch, m[r])
        if r - rounds < len(d):
            eng.push(1, d[r - rounds])
        eng.run()
        r += 1
    eng.flush()
    _compare(eng, 1, kind, rd, 'the reopened channel vs a fresh oracle')
    _compare(eng, 0, kind, r0, 'neighbour 0')
    _compare(eng, 2, kind, r2, 'neighbour 2')
    eng.close()


def _batch_variant(kind, k, phase):
    """the kind of channel k before (phase 0) and after (phase 1) the batch of
    closes; a burst MSK slot comes back at the other bit rate, whose scalar
    init differs"""
    if kind != 'burst_msk':
        return _kinds()[kind]
    br = 1200 if (k + phase) % 2 == 0 else 600
    return dict(open=dict(bitrate=br, fs=48000, burst=True), sizes=[12000], fs=None, sec_d=8.0,
                synth=lambda seed, sec, k: tl.synth_burst_msk(seconds=sec, bitrate=br, seed=seed,
                                                              carrier=2000.0 + 250.0 * k, ebn0=14.0),
                oracle=lambda: tl.Oracle(bitrate=br, burst=True))


BATCH_CLOSED = [1, 2, 4, 7]  # neighbours, a lone slot, the last one; 0, 3, 5, 6 stay
SEC_B = 3.0


@pytest.mark.parametrize('kind', ['oqpsk', 'c8400', 'burst_msk'])
def test_batch_of_closes_is_one_reset_launch(engine_lib, cpu_libs, kind):
    """Several slots closed before one run, neighbours and scattered: one
    launch of the reset kernel over the sorted slot list; every reopened
    channel equals a fresh oracle and every channel that stayed its own."""
    import aero_engine as ae
    flags = _kinds()['burst_msk1200' if kind == 'burst_msk' else kind]['flags']
    n = 8
    V0 = [_batch_variant(kind, k, 0) for k in range(n)]
    V1 = {k: _batch_variant(kind, k, 1) for k in BATCH_CLOSED}
    a, d, jobs = [], {}, {}
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        for k in range(n):
            sec = SEC_B if k in BATCH_CLOSED else SEC_B + V0[k]['sec_d']
            a.append(_messages(V0[k]['synth'](0xC1E000 + 8 * k, sec, k), V0[k]['sizes'], k))
            if k not in BATCH_CLOSED:
                jobs[k] = ex.submit(_reference, kind, a[k], V0[k])
        for k in BATCH_CLOSED:
            d[k] = _messages(V1[k]['synth'](0xC1E004 + 8 * k, V1[k]['sec_d'], k), V1[k]['sizes'], k + 3)
            jobs[k] = ex.submit(_reference, kind, d[k], V1[k])
        refs = {k: j.result() for k, j in jobs.items()}
    assert all(len(refs[k]['soft']) > 1000 for k in range(n)), 'an oracle did not lock'
    assert sum(_produced(kind, refs[k]) for k in BATCH_CLOSED) >= 2, 'the reopened channels decode too little'
    eng = ae.Engine(max_channels=n, flags=flags)
    assert [eng.open_channel(**V0[k]['open']) for k in range(n)] == list(range(n))
    rounds = min(len(a[k]) for k in BATCH_CLOSED)
    for r in range(rounds):
        for k in range(n):
            eng.push(k, a[k][r])
        eng.run()
    before = eng.stat('slot_resets')
    for k in (4, 1, 7, 2):  # not in slot order: the launch sorts them
        eng.close_channel(k)
    assert [eng.open_channel(**V1[k]['open']) for k in BATCH_CLOSED] == BATCH_CLOSED
    assert eng.stat('slot_resets') == before, 'a close or an open launched the reset by itself'
    r = rounds
    while any(r < len(a[k]) for k in range(n) if k not in BATCH_CLOSED) or any(r - rounds < len(d[k]) for k in d):
        for k in range(n):
            if k in BATCH_CLOSED:
                if r - rounds < len(d[k]):
                    eng.push(k, d[k][r - rounds])
            elif r < len(a[k]):
                eng.push(k, a[k][r])
        eng.run()
        r += 1
    eng.flush()
    assert eng.stat('slot_resets') == before + 1, 'the four slots were not reset by one launch'
    for k in range(n):
        _compare(eng, k, kind, refs[k], 'reopened channel %d' % k if k in BATCH_CLOSED else 'channel %d' % k)
    eng.close()


def test_rate_change_into_a_slot_awaiting_its_reset(engine_lib, cpu_libs, msk_kernel):
    """A leaves the 12 kHz group for 24 kHz (its slot's reset is queued), then
    B moves from 24 kHz into that slot before the 12 kHz group pushes or runs:
    the reset must be complete before B's state is written there."""
    import aero_engine as ae

    def msgs(segs, seed):
        out = []
        for i, (fs, sec) in enumerate(segs):
            x = tl.synth_msk(seconds=sec, bitrate=600, seed=seed + i, carrier=600.0, ebn0=14.0, fs=fs)
            step = fs // 4
            out += [(x[j:j + step], fs) for j in range(0, len(x), step)]
        return out
    ma = msgs([(12000, 4.0), (24000, 6.0)], 0xC1F0)
    mb = msgs([(24000, 4.0), (12000, 6.0)], 0xC1F8)
    refs = []
    for m in (ma, mb):
        o = tl.Oracle(bitrate=600)
        for pcm, fs in m:
            o.push(pcm, fs=fs)
        refs.append(o)
    eng = ae.Engine(max_channels=4, flags=ae.F_TRACE_SOFT | ae.F_TRACE_HOPS | ae.F_TRACE_FRAMES)
    A, B = eng.open_channel(600, fs=12000), eng.open_channel(600, fs=24000)
    assert len(ma) == len(mb)
    for (pa, fa), (pb, fb) in zip(ma, mb):
        eng.push(A, pa, fs=fa)  # at the rate change: A's 12 kHz slot is freed, its reset queued ...
        eng.push(B, pb, fs=fb)  # ... and B moves into it straight away
        eng.run()
    eng.flush()
    assert eng.stat('slot_resets') >= 1
    for ch, o in ((A, refs[0]), (B, refs[1])):
        sb, rsb = eng.softbits(ch), o.softbits()
        assert len(rsb) > 1000 and np.array_equal(sb, rsb), 'channel %d soft bits differ' % ch
        h, rh = eng.hops(ch), o.hops()
        assert h.shape == rh.shape and np.array_equal(h.view(np.int64), rh.view(np.int64)), ch
        assert np.array_equal(eng.frames(ch), o.frames()), ch
        assert eng.items(ch) == o.item_lines('A'), ch
    assert sum(len(o.frames()) for o in refs) >= 320
    eng.close()


@pytest.mark.parametrize('between', ['sync', 'close_neighbour'])
def test_drain_between_reopen_and_first_push(engine_lib, cpu_libs, between):
    """close(a); open() -> a; then a drain (aero_sync, or another channel's
    close) before the group pushes or runs again: the slot still
    holds the closed channel's device counters, and none of its soft bits or
    hops may reach the reopened channel, whose own must all arrive."""
    import aero_engine as ae
    K = _kinds()['oqpsk']
    a = [_messages(K['synth'](0xC1F100 + k, SEC_B if k else SEC_B + 6.0, k), K['sizes']) for k in range(3)]
    d = _messages(K['synth'](0xC1F108, 6.0, 3), K['sizes'])
    r0, rd = _reference('oqpsk', a[0]), _reference('oqpsk', d)
    assert _produced('oqpsk', r0) and _produced('oqpsk', rd)
    eng = ae.Engine(max_channels=3, flags=K['flags'])
    assert [eng.open_channel(**K['open']) for _ in range(3)] == [0, 1, 2]
    rounds = len(a[1])
    for r in range(rounds):
        for k in range(3):
            eng.push(k, a[k][r])
        eng.run()
    eng.close_channel(1)
    assert eng.open_channel(**K['open']) == 1
    before = eng.stat('slot_resets')
    if between == 'sync':
        eng.sync()
    else:
        eng.close_channel(2)
    assert eng.stat('slot_resets') == before  # (nothing has reset the slot yet)
    assert len(eng.softbits(1)) == 0 and len(eng.hops(1)) == 0, 'the closed channel leaked into the reopened one'
    for r in range(rounds, len(a[0])):
        eng.push(0, a[0][r])
        eng.push(1, d[r - rounds])
        eng.run()
    eng.flush()
    _compare(eng, 1, 'oqpsk', rd, 'the reopened channel vs a fresh oracle')
    _compare(eng, 0, 'oqpsk', r0, 'neighbour 0')
    eng.close()


def test_closed_id_is_invalid(engine_lib, cpu_libs):
    import aero_engine as ae
    L = engine_lib
    pcm = tl.synth(seconds=9.0, seed=0xC1A0, carrier=12037.5, ebn0=14.0)
    o = tl.Oracle()
    o.push_chunked(pcm, 12000)
    assert len(o.item_lines('A')) >= 2
    eng = ae.Engine(max_channels=4, flags=ae.F_TRACE_SOFT | ae.F_TRACE_FRAMES)
    chans = [eng.open_channel(10500, 48000) for _ in range(2)] + [eng.open_channel(10500, 48000, burst=True)]
    for i in range(0, len(pcm), 12000):
        eng.push(0, pcm[i:i + 12000])
        eng.push(1, pcm[i:i + 12000])
        eng.push(2, pcm[i:i + 12000])
        eng.run()
    eng.flush()  # channel 1's items are waiting in aero_pop_items_all
    eng.close_channel(1)
    eng.close_channel(2)
    got = eng.drain_items(lines=True)
    assert {c for c, _ in got} == {0} and [l for _, l in got] == o.item_lines('A')
    buf = np.zeros(4096, dtype=np.int16)
    n = ctypes.c_size_t()
    v64 = ctypes.c_int64()
    ev = ae.ChannelEvents()
    item = (ae.AcarsItem * 1)()
    one = (ctypes.c_int * 1)(1)
    dev = None
    for ch in (1, 2):
        pops = [L.aero_pop_softbits, L.aero_pop_hops, L.aero_pop_pt, L.aero_pop_blocks, L.aero_pop_frames,
                L.aero_pop_rt_tests, L.aero_pop_rt_packets, L.aero_pop_c_units, L.aero_pop_voice]
        for fn in pops:
            assert fn(eng.h, ch, buf.ctypes.data, 16, ctypes.byref(n)) == ae.AERO_E_INVALID, (fn.__name__, ch)
        assert L.aero_pop_items(eng.h, ch, item, 1, ctypes.byref(n)) == ae.AERO_E_INVALID
        assert L.aero_push_pcm(eng.h, ch, buf.ctypes.data, 4096, 48000) == ae.AERO_E_INVALID
        assert L.aero_push_pcm_dev(eng.h, ch, dev, 0, 48000) == ae.AERO_E_INVALID
        assert L.aero_channel_stat(eng.h, ch, b'hunter_scans', ctypes.byref(v64)) == ae.AERO_E_INVALID
        assert L.aero_channel_get_events(eng.h, ch, ctypes.byref(ev)) == ae.AERO_E_INVALID
        assert L.aero_channel_close(eng.h, ch) == ae.AERO_E_INVALID
    assert L.aero_trace_select(eng.h, one, 1) == ae.AERO_E_INVALID
    assert L.aero_push_pcm_batch(eng.h, buf.ctypes.data, 64, 2, 2, 0) == ae.AERO_E_INVALID  # channel 1 is closed
    # the channeliser's feed with the closed id: refused, nothing fed
    cfg = tl.PUB_CONFIGS['r288k']
    chan = ae.Channeliser(cfg['sample_rate'], tl.CENTER, cfg['mains'], cfg['vfos'][:1], max_blocks=1)
    x = tl.wideband(cfg['sample_rate'], chan.block_len, 0xC1A1, cfg['tones'])
    chan.push(x)
    chan.run()
    before = eng.samples_processed()
    with pytest.raises(ae.AeroError) as ei:
        chan.feed(eng, [1])
    assert ei.value.rc == ae.AERO_E_INVALID
    eng.flush()
    assert eng.samples_processed() == before
    chan.feed(eng, [0])  # the open channel still takes it
    eng.flush()
    assert eng.samples_processed() > before
    chan.close()
    eng.close()


def test_id_and_slot_order(engine_lib, cpu_libs):
    import aero_engine as ae
    eng = ae.Engine(max_channels=8, flags=ae.F_TRACE_SOFT)
    assert [eng.open_channel(10500, 48000) for _ in range(4)] == [0, 1, 2, 3]
    eng.close_channel(2)
    eng.close_channel(0)
    assert [eng.open_channel(10500, 48000) for _ in range(3)] == [0, 2, 4]
    streams = [tl.synth(seconds=2.0, seed=0xC1B0 + k, carrier=9000.0 + 1000.0 * k, ebn0=14.0) for k in range(4)]
    x = np.stack(streams, axis=1)
    for t in range(0, len(x), 12000):
        eng.push_batch(x[t:t + 12000], nch=4)  # engine channel j is still slot j
        eng.run()
    eng.flush()
    for k in range(4):
        o = tl.Oracle()
        o.push_chunked(streams[k], 12000)
        assert len(o.softbits()) > 1000 and np.array_equal(eng.softbits(k), o.softbits()), k
    eng.close()


def test_reserve_sizes_the_group(engine_lib):
    import aero_engine as ae
    small = ae.Engine(max_channels=4)
    small.open_channel(8400)
    want = small.stat('device_bytes')
    small.close()
    eng = ae.Engine(max_channels=4096)
    eng.reserve(4, bitrate=8400)
    eng.open_channel(8400)
    assert eng.stat('device_bytes') == want and eng.stat('groups') == 1
    with pytest.raises(ae.AeroError) as ei:
        eng.reserve(8, bitrate=8400)  # the group exists
    assert ei.value.rc == ae.AERO_E_INVALID
    for bad in (dict(n=0, bitrate=600), dict(n=4097, bitrate=600), dict(n=4, bitrate=9600),
                dict(n=4, bitrate=10500, fs=44100)):
        with pytest.raises(ae.AeroError) as ei:
            eng.reserve(**bad)
        assert ei.value.rc == ae.AERO_E_INVALID, bad
    eng.close()


@pytest.mark.parametrize('kind', [dict(bitrate=8400), dict(bitrate=10500, burst=True)], ids=['c8400', 'burst_oqpsk'])
def test_reserved_pool_is_full_at_its_size(engine_lib, kind):
    import aero_engine as ae
    eng = ae.Engine(max_channels=4096)
    eng.reserve(64, **kind)
    chans = [eng.open_channel(**kind) for _ in range(64)]
    assert chans == list(range(64))
    with pytest.raises(ae.AeroError) as ei:
        eng.open_channel(**kind)
    assert ei.value.rc == ae.AERO_E_FULL
    eng.close_channel(17)
    assert eng.open_channel(**kind) == 17
    with pytest.raises(ae.AeroError) as ei:
        eng.open_channel(**kind)
    assert ei.value.rc == ae.AERO_E_FULL
    eng.close()


def test_churn_in_a_reserved_pool(engine_lib, cpu_libs):
    import aero_engine as ae
    pcm = tl.synth_c(seconds=6.0, seed=0xC1C0, carrier=11000.0, ebn0=12.0)
    msgs = _messages(pcm, [12000])
    quiet = tl.synth_c(seconds=1.0, seed=0xC1C1, carrier=9000.0, ebn0=6.0)
    o = tl.Oracle(bitrate=8400)
    for m in msgs:
        o.push(m)
    eng = ae.Engine(max_channels=4096, flags=ae.F_TRACE_SOFT | ae.F_TRACE_FRAMES)
    eng.reserve(64, bitrate=8400)
    chans = [eng.open_channel(8400) for _ in range(64)]
    size, groups = eng.stat('device_bytes'), eng.stat('groups')
    for rnd in range(3):
        for ch in chans:  # every slot carries state when it is closed
            eng.push(ch, quiet[:12000])
        eng.run()
        victims = chans[5 + rnd:5 + rnd + 32:2]
        assert len(victims) == 16
        for ch in victims:
            eng.close_channel(ch)
        assert sorted(eng.open_channel(8400) for _ in victims) == victims
        assert (eng.stat('device_bytes'), eng.stat('groups')) == (size, groups)
        assert eng.stat('slot_resets') == rnd  # this round's 16 slots go in one launch, at the next push
    ch = victims[3]
    for m in msgs:
        eng.push(ch, m)
        eng.run()
    eng.flush()
    assert eng.stat('slot_resets') == 3
    assert len(o.softbits()) > 1000 and len(o.frames()) >= 320
    assert np.array_equal(eng.softbits(ch), o.softbits())
    assert np.array_equal(eng.frames(ch), o.frames())
    assert np.array_equal(eng.c_units(ch), o.c_units()) and eng.voice(ch) == o.voice()
    eng.close()


def test_last_close_releases_a_generic_group(engine_lib, cpu_libs):
    import aero_engine as ae
    # (a carrier the hunter finds at once: 8 s then hold a whole frame)
    pcm = tl.synth_msk(seconds=8.0, bitrate=600, seed=1, carrier=600.0, ebn0=14.0, fs=16000)
    eng = ae.Engine(max_channels=8)
    ch = eng.open_channel(600, fs=16000)
    for i in range(0, len(pcm), 4000):
        eng.push(ch, pcm[i:i + 4000])
        eng.run()
    eng.flush()
    jobs, frames = eng.stat('viterbi_jobs'), eng.stat('frames')
    assert eng.stat('groups') == 1 and jobs > 0 and frames > 0
    eng.close_channel(ch)
    assert eng.stat('groups') == 0
    assert eng.stat('viterbi_jobs') >= jobs and eng.stat('frames') >= frames
    eng.close()
