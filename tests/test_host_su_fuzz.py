"""PChannelHost (aero-cli_amd/csrc/acars_host.cpp through
tools/libaero_hostcheck.so) against the oracle past the modem
(oracle_feed_frame / oracle_feed_rt_packet / oracle_feed_isu_reset), on the
curated information fields of tests/frame_inputs.py and on seeded random
frames and R/T packets drawn from its SU grammar: random CRC masks and format
ids, reassembly on and off, isu_reset at random points.  The items must be
equal line for line.

The oracle alone shows that the inputs are not vacuous: every branch of the SU
dispatch and every return of ISUData::update, ParserISU::parse,
ACARSDefragmenter::defragment and RISUData::update is taken
(oracle_branch_hits), with at least 100 ACARS, 20 defragmented and 20
non-ACARS items.

The events are also written as a corpus for tools/hostfuzz_main.cpp, the
stand-alone sanitizer replay (AERO_HOSTFUZZ_CORPUS names the file to keep)."""
import ctypes
import os
import struct

import numpy as np
import pytest

import aero_engine as ae
import aero_testlib as tl
import frame_inputs as fi

SO = os.environ.get('AERO_HOSTCHECK_SO') or os.path.join(tl.ROOT, 'tools', 'libaero_hostcheck.so')
N_FRAMES, N_PACKETS = 2000, 500


@pytest.fixture(scope='module')
def hc(cpu_libs):
    if not os.environ.get('AERO_HOSTCHECK_SO'):
        import build
        build.build_hostcheck()
    L = ctypes.CDLL(SO)
    L.hc_create.restype = ctypes.c_void_p
    L.hc_destroy.argtypes = [ctypes.c_void_p]
    L.hc_isu_reset.argtypes = [ctypes.c_void_p]
    L.hc_frame.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_int]
    L.hc_rt_packet.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    L.hc_items.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    L.hc_items.restype = ctypes.c_size_t
    return L


def _items(L, h):
    arr = (ae.AcarsItem * 256)()
    out = []
    while True:
        n = L.hc_items(h, arr, 256)
        out += [ae.item_line(arr[i]) for i in range(n)]
        if n < 256:
            return out


# ------------------------------------------------------------------ inputs
def curated_frames():
    """the information fields of every 10500-bps class (lead and tail included), with their format ids"""
    ev = []
    for name in fi.P_CLASSES:
        for info, edit in fi.stream('p10500', name).frames:
            ev.append(('frame', info, (edit or {}).get('format', 1)))
        ev.append(('reset',))
    return ev


def _spoil(rng, su):
    """an SU with its CRC broken in one of the ways of frame_inputs.make_su"""
    how = ('bad', 'zero', 'swap')[int(rng.integers(3))]
    try:
        return fi.make_su(su[:10], how)
    except AssertionError:
        return fi.make_su(su[:10], 'bad')


def random_frames(n, seed):
    g = fi.Grammar(21, seed)
    rng = g.rng
    ev, pending = [], []
    while sum(e[0] == 'frame' for e in ev) < n:
        while len(pending) < 26:
            u = rng.random()
            if u < 0.30:
                pending += g.acars()
            elif u < 0.38:  # a more-to-come chain of two or three blocks, sometimes broken
                k = 2 + int(rng.integers(2))
                kw = dict(aes=g.aes[int(rng.integers(8))], ges=0x80 + int(rng.integers(4)), reg='.F-%04u' % rng.integers(4),
                          label=('H1', 'SA')[int(rng.integers(2))])
                first = 'ABXYZ'[int(rng.integers(5))]
                for j in range(k):
                    bi = chr((ord(first) - 65 + j + (rng.random() < 0.1)) % 26 + 65)
                    pending += g.acars(g.text(int(rng.integers(1, 12))), bi=bi, more=j < k - 1,
                                       tak=0x15 if rng.random() < 0.9 else 0x31, **kw)
            elif u < 0.46:
                bad = (int(rng.integers(4, 11)),) if rng.random() < 0.5 else (16 + int(rng.integers(4)),)
                pending += g.acars(g.text(8), bad=bad)
            elif u < 0.52:
                pending += fi.isu_chain(g.aes[int(rng.integers(8))] if rng.random() < 0.8 else 0, 0x80 + int(rng.integers(4)),
                                        int(rng.integers(16)), int(rng.integers(16)), bytes(g.rand(int(rng.integers(2, 40)))),
                                        rng, nooct=int(rng.integers(16)) if rng.random() < 0.3 else None,
                                        seqno=int(rng.integers(64)) if rng.random() < 0.2 else None)
            elif u < 0.58:
                pending += fi.isu_chain(g.aes[0], 0x81, int(rng.integers(16)), int(rng.integers(16)),
                                        fi.acars_ud(text=['A', 0x7F, 'B'], stx=rng.random() < 0.8), rng)
            elif u < 0.70:
                pending.append(g.typed((0x11, 0x21, 0x31, 0x32, 0x33, 0x34)[int(rng.integers(6))]))
            elif u < 0.76:
                pending.append(fi.make_su([0xC0 | int(rng.integers(64)), int(rng.integers(256))] + g.rand(8)))
            elif u < 0.80:
                pending.append(fi.ZERO_SU)
            elif u < 0.90:
                pending.append(g.typed(int(rng.integers(256))))
            else:
                pending.append(g.fill())
        # shuffled a little: SSUs out of order, ISUs between
        if rng.random() < 0.15:
            i = int(rng.integers(25))
            pending[i], pending[i + 1] = pending[i + 1], pending[i]
        nsu = 26 if rng.random() < 0.8 else int(rng.integers(0, 27))
        sus, pending = pending[:nsu], pending[nsu:]
        p_bad = (0.0, 0.05, 0.5)[int(rng.integers(3))]
        sus = [_spoil(rng, s) if rng.random() < p_bad else s for s in sus]
        info = b''.join(sus)
        if rng.random() < 0.05:
            info = info[:max(0, len(info) - int(rng.integers(1, 12)))]  # a ragged length: the rest is no SU
        ev.append(('frame', info, 1 if rng.random() < 0.7 else int(rng.integers(16))))
        if rng.random() < 0.03:
            ev.append(('reset',))
    return ev


def _r_packet(b0, b1, aes, ges, data, rng):
    ten = [b0, b1, (aes >> 16) & 255, (aes >> 8) & 255, aes & 255, ges] + list(data) + [int(v) for v in rng.integers(0, 256, 11)]
    ten = bytes(ten[:17])
    c = fi.crc16(ten)
    return ten + bytes([c & 255, c >> 8])


def random_packets(n, seed):
    """R packets (RISUData::update's sequence indicator / SU type combinations,
    the out-of-range write that grows userdata included) and T packets (ISU +
    SSUs behind a 6-byte header, whole and truncated)"""
    g = fi.Grammar(22, seed)
    rng = g.rng
    ev = []
    while len(ev) < n:
        u = rng.random()
        aes, ges = g.aes[int(rng.integers(4))], 0x80 + int(rng.integers(2))
        if u < 0.25:  # one ACARS message over three R packets, sometimes one missing or out of order
            ud = fi.acars_ud(reg='.R-%03u' % rng.integers(4), text=g.text(int(rng.integers(4, 9))))
            ud = ud[:33]
            key = (int(rng.integers(16)) << 4) | 0x08 | int(rng.integers(8))
            parts = [(4 + k, ud[11 * k:11 * k + 11]) for k in range(3)]
            if rng.random() < 0.2:
                parts.pop(int(rng.integers(3)))
            if rng.random() < 0.2:
                parts.reverse()
            for si, d in parts:
                ev.append(('rt', 'R', _r_packet((si << 4) | len(d), key, aes, ges, d, rng), 0))
        elif u < 0.60:  # any sequence indicator and SU type
            b0 = (int(rng.integers(16)) << 4) | int(rng.integers(16))
            b1 = (int(rng.integers(16)) << 4) | (0x08 if rng.random() < 0.9 else 0) | int(rng.integers(3))
            ev.append(('rt', 'R', _r_packet(b0, b1, aes if rng.random() < 0.9 else 0, ges, g.rand(11), rng), 0))
        else:  # T packet
            sus = g.acars() if rng.random() < 0.7 else fi.isu_chain(aes, ges, 1, 2, bytes(g.rand(int(rng.integers(2, 30)))), rng)
            if rng.random() < 0.2:
                sus.pop(int(rng.integers(len(sus))))
            hdr = bytes([(aes >> 16) & 255, (aes >> 8) & 255, aes & 255, ges])
            c = fi.crc16(hdr)
            pkt = hdr + bytes([c & 255, c >> 8]) + b''.join(sus)
            pkt = pkt[:-1]  # the reference chops the last byte
            nsus = len(sus)
            if rng.random() < 0.15:  # truncated: fewer bytes than the SU count promises
                pkt = pkt[:max(6, len(pkt) - int(rng.integers(1, 40)))]
            ev.append(('rt', 'T', pkt, nsus))
    return ev[:n]


# ------------------------------------------------------------------ the two sides
def oracle_side(events, burst=False):
    o = tl.Oracle(burst=burst)
    for e in events:
        if e[0] == 'frame':
            o.feed_frame(e[1], e[2])
        elif e[0] == 'reset':
            o.feed_isu_reset()
        else:
            kind, info, nsus = e[1:]
            if kind == 'T':
                # the reference never hands over a T packet shorter than its SU count says
                # (decode/aerol.h:816-830); PChannelHost stops at the first SU that does not fit
                # (acars_host.cpp rt_packet), which equals the whole SUs the bytes hold
                nsus = min(nsus, max(0, (len(info) - 6 + 2) // 12))
            assert o.feed_rt_packet(kind, info, nsus)
    return o


def host_side(hc, events, masks, disable):
    h = hc.hc_create(disable)
    k = 0
    for e in events:
        if e[0] == 'frame':
            hc.hc_frame(h, e[1], len(e[1]), masks[k], e[2])
            k += 1
        elif e[0] == 'reset':
            hc.hc_isu_reset(h)
        else:
            hc.hc_rt_packet(h, int(e[1] == 'R'), e[2], len(e[2]), e[3])
    got = _items(hc, h)
    hc.hc_destroy(h)
    return got


def write_corpus(path, runs):
    """runs: [(disable, events, masks)] -> the file tools/hostfuzz_main.cpp replays"""
    with open(path, 'wb') as f:
        f.write(b'AEROHF01')
        for disable, events, masks in runs:
            f.write(struct.pack('<BB', ord('N'), disable))
            k = 0
            for e in events:
                if e[0] == 'frame':
                    f.write(struct.pack('<BHIB', ord('F'), len(e[1]), masks[k], e[2]) + e[1])
                    k += 1
                elif e[0] == 'reset':
                    f.write(b'Z')
                else:
                    f.write(struct.pack('<BBHH', ord('P'), ord(e[1]), len(e[2]), e[3]) + e[2])


@pytest.fixture(scope='module')
def inputs(cpu_libs):
    frames = curated_frames() + random_frames(N_FRAMES, 1)
    packets = random_packets(N_PACKETS, 2)
    return frames, packets


def test_inputs_reach_every_branch(inputs):
    frames, packets = inputs
    assert sum(e[0] == 'frame' for e in frames) >= N_FRAMES + 100 and len(packets) >= N_PACKETS
    o, r = oracle_side(frames), oracle_side(packets, burst=True)
    hits, rhits = o.branch_hits(), r.branch_hits()
    for name in tl.BRANCHES:
        side = rhits if name.startswith('risu') else hits
        assert side[name] >= 1, '%s is never taken' % name
    for name in ('isu_new', 'ssu_last', 'ssu_missing', 'parse_acars', 'parse_nonacars'):
        assert rhits[name] >= 1, 'T packets: %s is never taken' % name
    a = o.item_lines('A')
    assert sum(' nonacars=0' in l for l in a) >= 100 and sum(' nonacars=1' in l for l in a) >= 20
    assert hits['defrag_joined'] >= 20, 'defragmented items'
    assert sum(m != (1 << 26) - 1 and m != 0 for _, m in tl.frame_records(o.frames())) >= 500, 'mixed masks'
    assert len(r.item_lines('A')) >= 50


@pytest.mark.parametrize('disable', [0, 1], ids=['reassembly', 'fragments'])
def test_frames_equal_oracle(hc, inputs, disable, tmp_path_factory):
    frames, _ = inputs
    o = oracle_side(frames)
    masks = [m for _, m in tl.frame_records(o.frames())]
    assert len(masks) == sum(e[0] == 'frame' for e in frames)
    got = host_side(hc, frames, masks, disable)
    ref = o.item_lines('F' if disable else 'A')
    assert len(ref) > 100
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g == r, 'item %d' % k
    assert len(got) == len(ref)


@pytest.mark.parametrize('disable', [0, 1], ids=['reassembly', 'fragments'])
def test_packets_equal_oracle(hc, inputs, disable):
    _, packets = inputs
    o = oracle_side(packets, burst=True)
    got = host_side(hc, packets, [], disable)
    ref = o.item_lines('F' if disable else 'A')
    assert len(ref) > 20
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g == r, 'item %d' % k
    assert len(got) == len(ref)


def test_corpus_for_the_sanitizer_replay(inputs, tmp_path):
    """the corpus tools/hostfuzz_main.cpp replays (build.py --hostfuzz builds it with ASan + UBSan)"""
    frames, packets = inputs
    o = oracle_side(frames)
    masks = [m for _, m in tl.frame_records(o.frames())]
    path = os.environ.get('AERO_HOSTFUZZ_CORPUS') or str(tmp_path / 'hostfuzz.corpus')
    write_corpus(path, [(d, ev, mk) for d in (0, 1) for ev, mk in ((frames, masks), (packets, []))])
    assert os.path.getsize(path) > 300 * N_FRAMES
