"""aero_channel_export / aero_channel_import on the GPU.

A live channel moves between two engines whose groups differ in size (so the
column pitch of every time-major array differs) and lands in another slot:
what the source delivered before its close, followed by what the destination
delivers, is bit for bit what one oracle emits for the uninterrupted stream,
for every channel kind, with samples pushed and not yet demodulated at the
export.  Every byte of the slot travels through the pack / unpack kernels
(csrc/slot_copy.hip) over the reset plan, so a per-channel array the plan
missed, or a host counter the blob missed, shows here as a moved channel that
differs from its oracle.  Then: an export is a snapshot (the source carries
on; one blob imports twice), a batch is one launch per group, refusals leave
no trace, and a blob written to a file continues in another process.

The streams are those of tests/test_gpu_channel_close.py (6 s before the
split: the 4-s AGC ring full, the loops locked, a frame in flight; 8 and 10 s
for the 1200- and 600-bps MSK kinds, whose first frame ends later: MOVED)."""
import concurrent.futures as cf
import ctypes
import functools
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_channel_close as cc

pytestmark = pytest.mark.gpu

# Per kind: the seed offset of the moved channel's stream and the seconds
# before the split, chosen on the CPU (the oracle alone) so that a frame (an
# R/T packet) is delivered both before and after the split, also by the
# engine, whose last run lies one message and up to a hop before the export.
# At 600 bps a frame lasts 2 s and none is complete 6 s into any stream tried
# (seed offsets 1, 4, 5, 6; the first comes after 7 to 8 s), and at 1200 bps
# the first ends in the last message before 6 s: those kinds split after 10 s
# and 8 s, with a frame well before the split.
MOVED = {'oqpsk': (1, cc.SEC_A), 'msk600': (1, 10.0), 'msk1200': (4, 8.0), 'msk600_16000': (1, 10.0),
         'c8400': (1, cc.SEC_A), 'burst_oqpsk': (4, cc.SEC_A), 'burst_msk1200': (1, cc.SEC_A)}


def _split(kind, msgs):
    """the rounds before the split: the messages that end within the kind's seconds"""
    rate = cc._kinds()[kind]['fs'] or 48000
    ends = np.cumsum([len(m) for m in msgs])
    return int(np.sum(ends <= MOVED[kind][1] * rate))


def _take(eng, ch, kind):
    """everything channel ch has to deliver now"""
    burst = 'burst' in kind
    out = dict(soft=eng.softbits16(ch) if burst else eng.softbits(ch), hops=eng.hops(ch))
    if burst:
        out.update(tests=eng.rt_tests(ch), packets=eng.rt_packets(ch))
    else:
        out.update(frames=eng.frames(ch))
    if kind == 'c8400':
        out.update(pt=eng.pt(ch), c_units=eng.c_units(ch), voice=eng.voice(ch))
    else:
        out.update(items=eng.items(ch))
    return out


def _join(a, b):
    return {k: (a[k] + b[k]) if isinstance(a[k], list) else np.concatenate([a[k], b[k]]) for k in a}


def _count(kind, got):
    return len(got['packets']) if 'burst' in kind else len(got['frames']) // 320


def _equal(got, events, kind, r, what):
    """`got` (source part + destination part) and the destination's event
    counters against the oracle of the whole stream"""
    burst = 'burst' in kind
    assert len(got['soft']) == len(r['soft']) and np.array_equal(got['soft'], r['soft']), '%s: soft bits' % what
    h = got['hops']
    assert h.shape == r['hops'].shape and np.array_equal(h.view(np.int64), r['hops'].view(np.int64)), \
        '%s: hop records' % what
    dcd, steps, fcs = events
    if burst:
        assert np.array_equal(got['tests'], r['tests']), '%s: R/T tests' % what
        assert got['packets'] == r['packets'], '%s: R/T packets' % what
        assert (dcd, steps) == (r['events'][0], 0), '%s: DCD changes' % what
    else:
        assert np.array_equal(got['frames'], r['frames']), '%s: frames' % what
        assert dcd == r['events'][0], '%s: DCD changes' % what
    if kind == 'c8400':
        assert got['pt'].shape == r['pt'].shape and \
            np.array_equal(got['pt'].view(np.int64), r['pt'].view(np.int64)), '%s: pt' % what
        assert np.array_equal(got['c_units'], r['c_units']), '%s: Call_progress SUs' % what
        assert got['voice'] == r['voice'], '%s: voice frames' % what
    else:
        assert got['items'] == r['items'], '%s: items' % what
        if not burst:
            assert steps == len(r['events'][1]) and fcs == r['events'][1][-8:], '%s: hunter steps' % what


@pytest.fixture(scope='module')
def move_refs(cpu_libs):
    """per kind: three channels' messages (0 and 2 stay; 1 moves) and their
    oracles over the whole streams; computed once"""
    out, jobs = {}, {}
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        for kind, K in sorted(cc._kinds().items()):
            total = MOVED[kind][1] + K['sec_d']
            seeds = [K['seed'], K['seed'] + MOVED[kind][0], K['seed'] + 2]
            a = [cc._messages(K['synth'](seeds[k], total, k), K['sizes'], k) for k in range(3)]
            out[kind] = dict(a=a)
            jobs[kind] = [ex.submit(cc._reference, kind, m) for m in a]
        for kind, js in jobs.items():
            out[kind]['refs'] = [j.result() for j in js]
    return out


@pytest.mark.parametrize('kind,shape', [('oqpsk', 'few'), ('oqpsk', 'one'), ('msk600', 'few'), ('msk600', 'one'),
                                        ('msk1200', 'few'), ('msk600_16000', 'few'), ('c8400', 'few'),
                                        ('burst_oqpsk', 'few'), ('burst_msk1200', 'few')])
def test_move_equals_uninterrupted(engine_lib, move_refs, monkeypatch, kind, shape):
    import aero_engine as ae
    cc._set_shape(monkeypatch, kind, shape)
    K = cc._kinds()[kind]
    a, refs = move_refs[kind]['a'], move_refs[kind]['refs']
    assert all(cc._produced(kind, r) for r in refs), 'an oracle produced too little'
    rounds = _split(kind, a[1])
    assert 0 < rounds < len(a[1]) - 2
    A = ae.Engine(max_channels=64, flags=K['flags'])
    B = ae.Engine(max_channels=128, flags=K['flags'])  # another column pitch
    assert [A.open_channel(**K['open']) for _ in range(3)] == [0, 1, 2]
    assert [B.open_channel(**K['open']) for _ in range(2)] == [0, 1]  # B's residents: the streams of A's 0 and 2
    res = {0: a[0], 1: a[2]}
    for r in range(rounds):
        for k in range(3):
            A.push(k, a[k][r])
        for j, m in res.items():
            B.push(j, m[r])
        A.run()
        B.run()
    # one more message without a run: a partial hop (continuous), a message
    # queued and not prefiltered (C), a message since the last run (burst)
    A.push(1, a[1][rounds])
    blob = A.export_channel(1)  # straight after: no sync
    head = _take(A, 1, kind)
    A.close_channel(1)
    ch = B.import_channel(blob)
    assert ch == 2, 'the import did not take the next id'
    r = rounds
    while r < max(len(a[0]), len(a[2]), len(a[1]) - 1):
        for k in (0, 2):
            if r < len(a[k]):
                A.push(k, a[k][r])
        for j, m in res.items():
            if r < len(m):
                B.push(j, m[r])
        if r + 1 < len(a[1]):
            B.push(ch, a[1][r + 1])
        A.run()
        B.run()
        r += 1
    A.flush()
    B.flush()
    tail = _take(B, ch, kind)
    print('%s/%s: blob %d bytes; frames or packets before %d, after %d' %
          (kind, shape, len(blob), _count(kind, head), _count(kind, tail)))
    assert _count(kind, head) >= 1 and _count(kind, tail) >= 1, 'the split does not fall between two frames'
    _equal(_join(head, tail), B.channel_events(ch), kind, refs[1], 'the moved channel')
    cc._compare(A, 0, kind, refs[0], "the source's neighbour 0")
    cc._compare(A, 2, kind, refs[2], "the source's neighbour 2")
    cc._compare(B, 0, kind, refs[0], "the destination's resident 0")
    cc._compare(B, 1, kind, refs[2], "the destination's resident 1")
    A.close()
    B.close()


@pytest.mark.parametrize('kind', ['oqpsk', 'burst_oqpsk'])
def test_export_is_a_snapshot(engine_lib, move_refs, kind):
    import aero_engine as ae
    K = cc._kinds()[kind]
    m, ref = move_refs[kind]['a'][1], move_refs[kind]['refs'][1]
    rounds = _split(kind, m)
    A = ae.Engine(max_channels=64, flags=K['flags'])
    B = ae.Engine(max_channels=128, flags=K['flags'])
    assert A.open_channel(**K['open']) == 0
    for r in range(rounds):
        A.push(0, m[r])
        A.run()
    blob = A.export_channel(0)
    head = _take(A, 0, kind)
    assert B.import_channels(blob + blob) == [0, 1], 'one blob, imported twice, is two channels'
    for r in range(rounds, len(m)):
        for eng, chans in ((A, [0]), (B, [0, 1])):
            for c in chans:
                eng.push(c, m[r])
            eng.run()
    A.flush()
    B.flush()
    # the source carried on as if nothing had happened
    _equal(_join(head, _take(A, 0, kind)), A.channel_events(0), kind, ref, 'the exported channel itself')
    t0, t1 = _take(B, 0, kind), _take(B, 1, kind)
    assert _count(kind, head) >= 1 and _count(kind, t0) >= 1
    _equal(_join(head, t0), B.channel_events(0), kind, ref, 'the first import')
    _equal(_join(head, t1), B.channel_events(1), kind, ref, 'the second import')
    A.close()
    B.close()


@pytest.mark.parametrize('kind', ['oqpsk', 'msk600', 'c8400'])
def test_y_travels_with_the_channel(engine_lib, move_refs, kind):
    """The coarse estimator's smoothed spectrum (aero_channel_coarse_y) read on
    the importing engine, in another slot of a group with another pitch,
    equals by bit pattern what the source read before the export."""
    import aero_engine as ae
    K = cc._kinds()[kind]
    m = move_refs[kind]['a'][1]
    A = ae.Engine(max_channels=64, flags=K['flags'])
    B = ae.Engine(max_channels=128, flags=K['flags'])
    assert A.open_channel(**K['open']) == 0
    assert [B.open_channel(**K['open']) for _ in range(3)] == [0, 1, 2]
    for r in range(min(12, _split(kind, m))):
        A.push(0, m[r])
        A.run()
    first, y = A.channel_coarse_y(0)
    assert y.max() > 20 and len(np.unique(y)) > 100, 'the channel has a history to carry'
    ch = B.import_channel(A.export_channel(0))
    assert ch == 3
    first_b, y_b = B.channel_coarse_y(ch)
    assert first_b == first and np.array_equal(y_b.view(np.int64), y.view(np.int64))
    _, y_res = B.channel_coarse_y(0)
    assert not y_res.any(), "a resident's row is untouched"
    with pytest.raises(ae.AeroError):
        B.channel_coarse_y(4)  # no such channel
    A.close()
    B.close()


BATCH_MOVED = [4, 1, 7, 2]  # not in slot order: neighbours, a lone slot, the last one


@functools.lru_cache(maxsize=None)
def _batch_refs(kind):
    n = 8
    V = [cc._batch_variant(kind, k, 0) for k in range(n)]
    a = [cc._messages(V[k]['synth'](0xC1E000 + 8 * k, cc.SEC_B + V[k]['sec_d'], k), V[k]['sizes'], k)
         for k in range(n)]
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        refs = list(ex.map(lambda k: cc._reference(kind, a[k], V[k]), range(n)))
    return V, a, refs


@pytest.mark.parametrize('pending', [False, True], ids=['free', 'reset_pending'])
@pytest.mark.parametrize('kind', ['oqpsk', 'c8400', 'burst_msk'])
def test_batch_is_one_launch_per_group(engine_lib, cpu_libs, kind, pending):
    """Four of eight channels, scattered, in one export and one import: one
    pack launch on the source, one unpack launch on the destination (also when
    the slots they land in were closed a moment ago and await their reset)."""
    import aero_engine as ae
    flags = cc._kinds()['burst_msk1200' if kind == 'burst_msk' else kind]['flags']
    n = 8
    V, a, refs = _batch_refs(kind)
    assert all(len(refs[k]['soft']) > 1000 for k in range(n)), 'an oracle did not lock'
    assert sum(cc._produced(kind, refs[k]) for k in BATCH_MOVED) >= 2, 'the moved channels decode too little'
    A = ae.Engine(max_channels=n, flags=flags)
    B = ae.Engine(max_channels=128, flags=flags)
    assert [A.open_channel(**V[k]['open']) for k in range(n)] == list(range(n))
    if pending:
        # four channels with state in B's slots 0..3, closed just before the import
        old = [B.open_channel(**V[k]['open']) for k in BATCH_MOVED]
        for c, k in zip(old, BATCH_MOVED):
            B.push(c, a[k][0])
        B.run()
    rate = 48000
    rounds = int(np.sum(np.cumsum([len(m) for m in a[0]]) <= cc.SEC_B * rate))
    assert 0 < rounds < min(len(m) for m in a)
    for r in range(rounds):
        for k in range(n):
            A.push(k, a[k][r])
        A.run()
    copies_a, copies_b, resets_b = A.stat('slot_copies'), B.stat('slot_copies'), B.stat('slot_resets')
    blob = A.export_channels(BATCH_MOVED)
    assert A.stat('slot_copies') == copies_a + 1, 'four channels of one group are one pack launch'
    heads = {k: _take(A, k, kind) for k in BATCH_MOVED}
    for k in BATCH_MOVED:
        A.close_channel(k)
    if pending:
        for c in old:
            B.close_channel(c)
        assert B.stat('slot_resets') == resets_b  # queued, not launched
    chans = B.import_channels(blob)
    assert chans == [0, 1, 2, 3], 'ids in blob order, the smallest first'
    assert B.stat('slot_copies') == copies_b + 1, 'four channels of one group are one unpack launch'
    assert B.stat('slot_resets') == resets_b + (1 if pending else 0)
    where = dict(zip(BATCH_MOVED, chans))
    for r in range(rounds, max(len(m) for m in a)):
        for k in range(n):
            if r < len(a[k]):
                (B if k in where else A).push(where.get(k, k), a[k][r])
        A.run()
        B.run()
    A.flush()
    B.flush()
    assert B.stat('slot_copies') == copies_b + 1 and A.stat('slot_copies') == copies_a + 1
    for k in range(n):
        if k in where:
            _equal(_join(heads[k], _take(B, where[k], kind)), B.channel_events(where[k]), kind, refs[k],
                   'moved channel %d' % k)
        else:
            cc._compare(A, k, kind, refs[k], 'channel %d, which stayed' % k)
    A.close()
    B.close()


def test_refusals_leave_no_trace(engine_lib, move_refs):
    import aero_engine as ae
    L = engine_lib
    K = cc._kinds()['oqpsk']
    m, ref = move_refs['oqpsk']['a'][0], move_refs['oqpsk']['refs'][0]
    src = move_refs['oqpsk']['a'][1]
    A = ae.Engine(max_channels=64, flags=K['flags'])
    B = ae.Engine(max_channels=128, flags=K['flags'])
    assert [A.open_channel(**K['open']) for _ in range(2)] == [0, 1]
    assert B.open_channel(**K['open']) == 0
    for r in range(4):
        A.push(0, src[r])
        A.run()
    half = len(m) // 2
    for r in range(half):
        B.push(0, m[r])
        B.run()
    A.close_channel(1)

    def state(eng):
        return eng.stat('device_bytes'), eng.stat('groups'), eng.stat('slot_copies')

    def untouched(eng, before, next_id, what):
        assert state(eng) == before, what
        c = eng.open_channel(**K['open'])
        assert c == next_id, '%s: the next id is %d, not %d' % (what, c, next_id)
        eng.close_channel(c)

    # ---- export ----
    sa = state(A)
    need = ctypes.c_size_t()
    buf = np.full(1 << 22, 0xEE, dtype=np.uint8)
    for bad in (1, 2, 64, -1):  # closed, never opened, out of range
        one = (ctypes.c_int * 1)(bad)
        assert L.aero_channel_export(A.h, one, 1, buf.ctypes.data, buf.size, ctypes.byref(need)) == \
            ae.AERO_E_INVALID, bad
    one = (ctypes.c_int * 1)(0)
    assert L.aero_channel_export(A.h, one, 1, None, 0, ctypes.byref(need)) == ae.AERO_OK  # the size query
    size = need.value
    assert 64 < size <= buf.size
    assert L.aero_channel_export(A.h, one, 1, buf.ctypes.data, size - 1, ctypes.byref(need)) == ae.AERO_E_FULL
    assert need.value == size and np.all(buf == 0xEE), 'a refused export wrote to the buffer'
    untouched(A, sa, 1, 'refused exports and the size query')
    blob = A.export_channel(0)
    assert len(blob) == size and A.stat('slot_copies') == sa[2] + 1

    # ---- import ----
    sb = state(B)
    out = (ctypes.c_int * 8)()
    k = ctypes.c_int()

    def imp(eng, data, cap=8):
        return L.aero_channel_import(eng.h, data, len(data), out, cap, ctypes.byref(k))

    dev_len, = struct.unpack_from('<Q', blob, 48)
    cases = {
        'truncated': blob[:-1],
        'truncated to the header': blob[:48],
        'bad magic': b'X' + blob[1:],
        'bad version': blob[:8] + struct.pack('<I', 2) + blob[12:],
        'total length too long': blob[:40] + struct.pack('<Q', len(blob) + 1) + blob[48:],
        'total length too short': blob[:40] + struct.pack('<Q', len(blob) - 1) + blob[48:],
        'device section past the end': blob[:48] + struct.pack('<Q', len(blob)) + blob[56:],
        'host section past the end': blob[:56 + dev_len] + struct.pack('<Q', 1 << 40) + blob[64 + dev_len:],
        'a kind open refuses': blob[:12] + struct.pack('<i', 9600) + blob[16:],
        'another kind': blob[:12] + struct.pack('<i', 8400) + blob[16:],
        'another fingerprint': blob[:32] + struct.pack('<Q', 1) + blob[40:],
        'a batch whose third blob is corrupt': blob + blob + blob[:100] + b'\x00' * (len(blob) - 100),
        'a batch with a cut third blob': blob + blob + blob[:len(blob) // 2],
    }
    for what, data in cases.items():
        assert imp(B, data) == ae.AERO_E_INVALID, what
        assert k.value == 0, what
        untouched(B, sb, 1, what)
    assert imp(B, blob + blob, cap=1) == ae.AERO_E_FULL
    untouched(B, sb, 1, 'more blobs than ids')
    # engines whose decode-shaping flags differ from the blob's
    for flags, what in ((K['flags'] & ~ae.F_DCD_TICK, 'no DCD tick'), (K['flags'] | ae.F_TRACE_PT, 'pt trace')):
        E = ae.Engine(max_channels=64, flags=flags)
        se = state(E)
        assert imp(E, blob) == ae.AERO_E_INVALID, what
        untouched(E, se, 0, what)
        E.close()
    # ... but AERO_F_TRACE_FRAMES does not shape the decode
    E = ae.Engine(max_channels=64, flags=K['flags'] & ~ae.F_TRACE_FRAMES)
    assert imp(E, blob) == ae.AERO_OK and k.value == 1 and out[0] == 0
    E.close()
    # a full reserved pool
    R = ae.Engine(max_channels=4096, flags=K['flags'])
    R.reserve(64, **K['open'])
    assert [R.open_channel(**K['open']) for _ in range(63)] == list(range(63))
    sr = state(R)
    assert imp(R, blob + blob) == ae.AERO_E_FULL
    untouched(R, sr, 63, 'a full reserved pool')
    assert imp(R, blob) == ae.AERO_OK and out[0] == 63
    assert imp(R, blob) == ae.AERO_E_FULL
    R.close()

    # B's running channel never noticed
    for r in range(half, len(m)):
        B.push(0, m[r])
        B.run()
    B.flush()
    cc._compare(B, 0, 'oqpsk', ref, "the destination's running channel")
    A.close()
    B.close()


CHILD = r'''
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import aero_engine as ae
blob = open(sys.argv[3], 'rb').read()
pcm = np.load(sys.argv[4])
eng = ae.Engine(max_channels=128, flags=int(sys.argv[6]))
ch = eng.import_channel(blob)
for i in range(0, len(pcm), 12000):
    eng.push(ch, pcm[i:i + 12000])
    eng.run()
eng.flush()
dcd, steps, fcs = eng.channel_events(ch)
np.savez(sys.argv[5], soft=eng.softbits(ch), hops=eng.hops(ch), frames=eng.frames(ch),
         items=np.frombuffer(json.dumps(eng.items(ch)).encode(), np.uint8),
         events=np.frombuffer(json.dumps([dcd, steps, fcs]).encode(), np.uint8))
eng.close()
'''


def test_restart_from_a_file(engine_lib, move_refs, tmp_path):
    """the parent writes the blob to a file and closes its engine; a new
    process imports it and decodes the rest"""
    import aero_engine as ae
    K = cc._kinds()['oqpsk']
    m, ref = move_refs['oqpsk']['a'][1], move_refs['oqpsk']['refs'][1]
    rounds = _split('oqpsk', m)
    A = ae.Engine(max_channels=64, flags=K['flags'])
    assert A.open_channel(**K['open']) == 0
    for r in range(rounds):
        A.push(0, m[r])
        A.run()
    blob_path, pcm_path, out_path = (str(tmp_path / n) for n in ('chan.blob', 'rest.npy', 'out.npz'))
    with open(blob_path, 'wb') as f:
        f.write(A.export_channel(0))
    head = _take(A, 0, 'oqpsk')
    A.close()
    np.save(pcm_path, np.concatenate(m[rounds:]))
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, '-c', CHILD, here, os.path.dirname(ae.__file__), blob_path, pcm_path, out_path,
                        str(K['flags'])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out_path)
    tail = dict(soft=z['soft'], hops=z['hops'], frames=z['frames'], items=json.loads(z['items'].tobytes().decode()))
    events = json.loads(z['events'].tobytes().decode())
    assert _count('oqpsk', head) >= 1 and _count('oqpsk', tail) >= 1
    _equal(_join(head, tail), tuple(events), 'oqpsk', ref, 'parent + child')
