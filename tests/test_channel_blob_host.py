"""Channel export / import, the parts that need no GPU.

* PChannelHost::save / load (csrc/chan_blob.cpp through tools/hostcheck.cpp):
  the ISU / R-ISU reassembly and the ACARS defragmenter's messages in flight
  travel, so a host saved at any frame or packet boundary and loaded into a
  new one goes on to emit what the uninterrupted host emits (the oracle's
  items); a truncated or mutated state is refused or taken, never a crash,
  and a host that refused one is a new host.
* The pack / unpack addressing (csrc/slot_copy.h through aero_x_slot_pack /
  aero_x_slot_unpack, the plain C++ the kernels of slot_copy.hip restate): a
  slot packed from a 64-channel pool and unpacked into a 128-channel pool
  lands byte for byte on what the plan gives the destination slot and
  nowhere else."""
import ctypes
import os

import numpy as np
import pytest

import aero_testlib as tl
import aero_engine as ae

SO = os.environ.get('AERO_HOSTCHECK_SO') or os.path.join(tl.ROOT, 'tools', 'libaero_hostcheck.so')


@pytest.fixture(scope='module')
def hc():
    if not os.environ.get('AERO_HOSTCHECK_SO'):
        import build
        build.build_hostcheck()
    L = ctypes.CDLL(SO)
    L.hc_create.restype = ctypes.c_void_p
    L.hc_destroy.argtypes = [ctypes.c_void_p]
    L.hc_frame.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_int]
    L.hc_rt_packet.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    L.hc_items.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.hc_items.restype = ctypes.c_size_t
    L.hc_save.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.hc_save.restype = ctypes.c_size_t
    L.hc_load.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    L.hc_load.restype = ctypes.c_int
    return L


_ARR = (ae.AcarsItem * 256)()


def _items(L, h):
    out = []
    while True:
        n = L.hc_items(h, _ARR, 256)
        out += [ae.item_line(_ARR[i]) for i in range(n)]
        if n < 256:
            return out


def _save(L, h):
    n = L.hc_save(h, None, 0)
    buf = ctypes.create_string_buffer(n)
    assert L.hc_save(h, buf, n) == n
    return buf.raw


def _feed(L, h, ev):
    """one frame ('F', info, mask) or R/T packet ('R' / 'T', info, nsus)"""
    if ev[0] == 'F':
        L.hc_frame(h, ev[1], len(ev[1]), ev[2], 1)
    else:
        L.hc_rt_packet(h, int(ev[0] == 'R'), ev[1], len(ev[1]), ev[2])


@pytest.fixture(scope='module')
def streams(cpu_libs):
    """the streams of tests/test_hostcheck.py as event lists, with the oracle's
    items reassembled ('A') and as fragments ('F')"""
    out = {}
    for name, bitrate, seed in (('oqpsk_ae20', 10500, 0xAE20), ('oqpsk_ae23', 10500, 0xAE23),
                                ('msk600_ae40', 600, 0xAE40)):
        if bitrate == 10500:
            pcm = tl.synth(seconds=20.0, seed=seed)
        else:
            pcm = tl.synth_msk(seconds=40.0, bitrate=600, baud=600, seed=seed, ebn0=14.0)
        o = tl.Oracle(bitrate=bitrate)
        o.push_chunked(pcm, 6000)
        ev = [('F', info, mask) for info, mask in tl.frame_records(o.frames())]
        out[name] = (ev, {0: o.item_lines('A'), 1: o.item_lines('F')})
    pcm = tl.synth_burst(seconds=30.0, seed=3, carrier=12000.0, ebn0=14.0)
    o = tl.Oracle(burst=True)
    o.push_chunked(pcm, 12000)
    ev = [(kind, info, max(0, (len(info) + 1 - 6) // 12) if kind == 'T' else 0) for kind, info in o.rt_packets()]
    out['burst_rt'] = (ev, {0: o.item_lines('A'), 1: o.item_lines('F')})
    return out


STREAMS = ['oqpsk_ae20', 'oqpsk_ae23', 'msk600_ae40', 'burst_rt']


def test_reassembly_state_travels(hc, streams):
    """save at every boundary, load into a new host, feed the rest: the items
    before plus the items after are the uninterrupted run's.  The streams
    exercise the state: somewhere the saved state is larger than a new host's,
    and somewhere going on in a new host without the load gives other items."""
    grew, differs = {}, {}
    for name in STREAMS:
        ev, refs = streams[name]
        assert len(ev) >= 3, name
        for disable in (0, 1):
            ref = refs[disable]
            assert ref, (name, disable)
            h0 = hc.hc_create(disable)
            fresh = len(_save(hc, h0))
            hc.hc_destroy(h0)
            for k in range(len(ev) + 1):
                a = hc.hc_create(disable)
                for e in ev[:k]:
                    _feed(hc, a, e)
                head = _items(hc, a)
                state = _save(hc, a)
                hc.hc_destroy(a)
                # (the target is made for the other setting: the state carries disable_reassembly)
                b = hc.hc_create(1 - disable)
                assert hc.hc_load(b, state, len(state)) == 1, (name, disable, k)
                assert _save(hc, b) == state, (name, disable, k)
                c = hc.hc_create(disable)
                for e in ev[k:]:
                    _feed(hc, b, e)
                    _feed(hc, c, e)
                tail, cold = _items(hc, b), _items(hc, c)
                hc.hc_destroy(b)
                hc.hc_destroy(c)
                assert head + tail == ref, (name, disable, k)
                if len(state) > fresh:
                    grew[(name, disable)] = grew.get((name, disable), 0) + 1
                if head + cold != ref:
                    differs[(name, disable)] = differs.get((name, disable), 0) + 1
    print('boundaries with state larger than a new host:', grew)
    print('boundaries where a new host goes on differently:', differs)
    assert grew, 'no boundary carries any state'
    assert any(k[1] == 0 for k in differs), 'the reassembly state never matters to the reassembled items'


def _busiest(hc, ev):
    """the boundary with the largest saved state: (events before, state)"""
    best = (0, b'')
    h = hc.hc_create(0)
    for k, e in enumerate(ev):
        _feed(hc, h, e)
        s = _save(hc, h)
        if len(s) > len(best[1]):
            best = (k + 1, s)
    hc.hc_destroy(h)
    return best


def test_malformed_state_is_refused(hc, streams):
    """every truncation and 2000 seeded one-byte mutations of a saved state
    with messages in flight: refused or taken, never a crash; a host that
    refused behaves as a new one"""
    ev, _ = streams['oqpsk_ae20']
    k, state = _busiest(hc, ev)
    h = hc.hc_create(0)
    fresh_len = len(_save(hc, h))
    assert len(state) > fresh_len + 16, 'the state holds nothing'
    tail = ev[k:] or ev[-3:]
    for e in tail:
        _feed(hc, h, e)
    fresh_items = _items(hc, h)
    fresh_after = _save(hc, h)
    hc.hc_destroy(h)

    def attempt(blob, what):
        h = hc.hc_create(0)
        # a host with something in it, so that "as a new one" is visible
        for e in ev[:k]:
            _feed(hc, h, e)
        _items(hc, h)
        ok = hc.hc_load(h, blob, len(blob))
        assert ok in (0, 1), what
        for e in tail:
            _feed(hc, h, e)
        got = _items(hc, h)
        if not ok:
            assert got == fresh_items and _save(hc, h) == fresh_after, what
        hc.hc_destroy(h)
        return ok

    assert attempt(state, 'whole') == 1
    refused = 0
    for n in range(len(state)):
        ok = attempt(state[:n], 'cut at %d' % n)
        assert ok == 0, 'a truncated state was taken (%d of %d bytes)' % (n, len(state))
        refused += 1
    rng = np.random.default_rng(0xB10B)
    taken = 0
    for i in range(2000):
        pos = int(rng.integers(0, len(state)))
        val = int(rng.integers(1, 256))
        m = bytearray(state)
        m[pos] ^= val
        taken += attempt(bytes(m), 'mutation %d: byte %d ^ %d' % (i, pos, val))
    print('truncations refused: %d; mutations taken: %d of 2000' % (refused, taken))
    assert 0 < taken < 2000  # a changed text byte is a state like any other; a changed length is not


# aero_x_reset_plan kinds (tests/test_channel_lifecycle_host.py): every kind of pool
MODE_MSKG600, MODE_C8400 = 8, 10
KINDS = {'oqpsk': 0, 'msk600': 1, 'msk1200': 2, 'mskg600_16000': MODE_MSKG600 | (16000 << 8), 'c8400': MODE_C8400,
         'burst_oqpsk': 100, 'burst_msk': 101}
TRACE = ae.F_TRACE_PT | ae.F_TRACE_BLOCKS | ae.F_TRACE_SOFT | ae.F_TRACE_HOPS


def _plan(L, kind, C, flags, slot):
    n = L.aero_x_reset_plan(kind, C, flags, slot, None, 0)
    assert n > 0
    out = np.zeros((n, 7), dtype=np.uint64)
    assert L.aero_x_reset_plan(kind, C, flags, slot, out.ctypes.data_as(ctypes.c_void_p), n) == n
    return [tuple(int(v) for v in r) for r in out]


def _slot_index(plan):
    """pool byte offsets of one slot, in packed order"""
    idx = []
    for start, elem, rows, pitch, kind, fill, total in plan:
        idx.append((start + np.arange(rows, dtype=np.int64)[:, None] * pitch + np.arange(elem, dtype=np.int64)).ravel())
    return np.concatenate(idx)


@pytest.mark.parametrize('flags', [0, TRACE], ids=['plain', 'trace'])
@pytest.mark.parametrize('name', sorted(KINDS))
def test_pack_unpack_addressing(engine_lib, name, flags):
    L = engine_lib
    L.aero_x_slot_pack.restype = ctypes.c_longlong
    L.aero_x_slot_unpack.restype = ctypes.c_longlong
    L.aero_x_slot_pack.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_void_p]
    L.aero_x_slot_unpack.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_void_p]
    kind = KINDS[name]
    size_a = _plan(L, kind, 64, flags, -1)[-1][0]
    size_b = _plan(L, kind, 128, flags, -1)[-1][0]
    # a byte pattern that is a function of the offset (two coprime periods, so shifted runs differ)
    off = np.arange(size_a, dtype=np.int64)
    pool_a = ((off % 251) * 7 + (off // 251) % 241 + 1).astype(np.uint8)
    pool_b = np.zeros(size_b, dtype=np.uint8)
    want_b = np.zeros(size_b, dtype=np.uint8)
    per_slot = sum(p[1] * p[2] for p in _plan(L, kind, 64, flags, 0))
    assert L.aero_x_slot_pack(kind, 64, flags, 0, None, None) == per_slot
    fp = [ctypes.c_uint64() for _ in range(3)]
    assert L.aero_x_plan_fingerprint(kind, 64, flags, ctypes.byref(fp[0])) == 0
    assert L.aero_x_plan_fingerprint(kind, 128, flags, ctypes.byref(fp[1])) == 0
    assert L.aero_x_plan_fingerprint(kind, 64, flags ^ ae.F_TRACE_PT, ctypes.byref(fp[2])) == 0
    assert fp[0].value == fp[1].value, 'the fingerprint depends on the channel count'
    if kind < 100:  # the trace arrays are the continuous pools'
        assert fp[0].value != fp[2].value, 'the fingerprint misses a trace array'
    for src, dst in ((0, 63), (17, 0), (63, 5)):
        blob = np.zeros(per_slot, dtype=np.uint8)
        assert L.aero_x_slot_pack(kind, 64, flags, src, pool_a.ctypes.data, blob.ctypes.data) == per_slot
        ia = _slot_index(_plan(L, kind, 64, flags, src))
        assert len(ia) == per_slot and np.array_equal(blob, pool_a[ia]), 'pack order (slot %d)' % src
        assert L.aero_x_slot_unpack(kind, 128, flags, dst, pool_b.ctypes.data, blob.ctypes.data) == per_slot
        ib = _slot_index(_plan(L, kind, 128, flags, dst))
        assert len(ib) == per_slot
        want_b[ib] = pool_a[ia]
        # every byte of the destination slot is the source slot's, and no other byte changed
        assert np.array_equal(pool_b, want_b), 'slot %d -> %d' % (src, dst)
        back = np.zeros(per_slot, dtype=np.uint8)
        assert L.aero_x_slot_pack(kind, 128, flags, dst, pool_b.ctypes.data, back.ctypes.data) == per_slot
        assert np.array_equal(back, blob), 'pack(unpack(blob)) != blob'
    assert np.count_nonzero(want_b) > 0.9 * 3 * per_slot
    for bad in ((kind, 63, 0), (kind, 64, 64), (kind, 64, -1), (7, 64, 0)):
        assert L.aero_x_slot_pack(bad[0], bad[1], flags, bad[2], pool_a.ctypes.data, None) < 0, bad


def test_null_arguments_are_invalid(engine_lib):
    L = engine_lib
    n = ctypes.c_size_t()
    k = ctypes.c_int()
    one = (ctypes.c_int * 1)(0)
    assert L.aero_channel_export(None, one, 1, None, 0, ctypes.byref(n)) == ae.AERO_E_INVALID
    assert L.aero_channel_import(None, b'x', 1, one, 1, ctypes.byref(k)) == ae.AERO_E_INVALID
