"""The coarse kernel's LDS map on the CPU (aero-cli_amd/csrc/coarse_lds.h
through tools/coarse_lds_sim.cpp) for the 16384-point kinds.

The overlapped head keeps the next channel's ring image in the hop's tail
behind ylds: over the rest of lds, all of s_tw and a spare.  Every word of
the image must lie inside that region, outside ylds's span and outside
red_* and the log table, no two words may share a place, and the whole must
fit one workgroup's 160 KiB.  A changed YLO/YHI, TwLds or padding that breaks
the overlay fails here (and in the header's static_asserts)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 14
N = 1 << L
YLEN = 13568 - 2815 + 1
NAMES = ['lds', 's_tw', 'spare', 'red_v', 'red_i', 'logtab', 'img']


@pytest.fixture(scope='module')
def sim():
    sys.path.insert(0, os.path.join(ROOT, 'aero-cli_amd'))
    import build
    lib = ctypes.CDLL(build.build_ldssim())
    lib.coarse_lds_regions.argtypes = [ctypes.c_int, ctypes.c_void_p]
    lib.coarse_lds_image.argtypes = [ctypes.c_void_p]
    lib.coarse_lds_ybin.argtypes = [ctypes.c_int]
    return lib


def _regions(sim, overlap):
    r = np.zeros(18, dtype=np.int32)
    sim.coarse_lds_regions(overlap, r.ctypes.data)
    reg = {n: (int(r[2 * k]), int(r[2 * k + 1])) for k, n in enumerate(NAMES)}
    return reg, int(r[14]), int(r[15]), int(r[16]), int(r[17])


def _image(sim):
    off = np.zeros(N, dtype=np.int32)
    sim.coarse_lds_image(off.ctypes.data)
    return off.astype(np.int64)


def test_total_and_carving(sim):
    for overlap in (1, 0):
        reg, y_bytes, total, limit, n = _regions(sim, overlap)
        assert n == N and limit == 163840
        assert total <= 163840
        carved = [reg[k] for k in NAMES[:6]]
        for (o0, s0), (o1, _) in zip(carved, carved[1:]):
            assert o0 + s0 <= o1, 'carved regions in order, not overlapping'
        assert carved[-1][0] + carved[-1][1] == total or not overlap
        assert reg['lds'] == (0, (N + N // 16) * 8)
        assert reg['s_tw'][1] == 1023 * 16 and reg['s_tw'][0] % 16 == 0
        assert y_bytes <= reg['lds'][1]
    plain = _regions(sim, 0)
    assert plain[0]['spare'][1] == 0 and plain[0]['logtab'][1] == 0
    assert plain[2] == 155824, 'the plain instances keep their footprint'


def test_ylds_span(sim):
    _, y_bytes, _, _, _ = _regions(sim, 1)
    offs = np.array([sim.coarse_lds_ybin(q) for q in range(YLEN)], dtype=np.int64)
    assert len(np.unique(offs)) == YLEN
    assert offs.min() == 0 and offs.max() + 8 == y_bytes


def test_image_inside_its_region_and_injective(sim):
    reg, y_bytes, total, _, _ = _regions(sim, 1)
    off = _image(sim)
    lo, size = reg['img']
    assert np.all(off % 4 == 0)
    assert off.min() >= lo and off.max() + 4 <= lo + size
    assert len(np.unique(off)) == N, 'no two ring words share a place'
    assert off.min() >= y_bytes, 'behind every y bin'
    for name in ('red_v', 'red_i', 'logtab'):
        o, s = reg[name]
        assert np.all((off + 4 <= o) | (off >= o + s)), 'clear of ' + name
    assert off.max() + 4 <= total


def test_image_covers_s_tw_whole(sim):
    """After the image is read the kernel writes all of s_tw again from the
    twiddle table (thread j entry j), so the image may lie over s_tw whole or
    stay clear of it, but must not end inside it."""
    reg, _, _, _, _ = _regions(sim, 1)
    lo, size = reg['img']
    two, tws = reg['s_tw']
    assert lo + size <= two or lo + size >= two + tws
    assert lo + size <= reg['red_v'][0]
    # and it needs the spare exactly as far as it reaches past s_tw
    assert reg['spare'][1] >= max(0, lo + size - (two + tws))


def test_bank_spread_of_the_bit_reversed_read(sim):
    """The gather reads words 16 apart (bit-reversed order): with one pad
    word per 16 the 64 lanes of a wave hit 64 different banks."""
    off = _image(sim)
    for base in (0, 5, 4096 + 3, N - 16 * 64):
        j = base + 16 * np.arange(64)
        assert len(np.unique((off[j] // 4) % 64)) == 64
