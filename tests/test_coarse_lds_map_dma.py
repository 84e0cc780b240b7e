"""The overlapped head's ring image as direct-to-LDS loads fill it
(aero-cli_amd/csrc/coarse_lds.h through tools/coarse_lds_sim.cpp), on the CPU.

A load that writes the LDS directly puts a wave's 64 words at a wave-uniform
base plus lane x 4, so the 64 places of every wave-load must be consecutive
words, in lane order.  The pad that keeps the bit-reversed read off the same
banks is therefore one word per 64 and no longer one per 16; the read set the
kernel really makes (thread t, element i, snapshot start s0:
q = (s0 + bitrev14(16 t + i)) & 16383) must stay within a 2-way conflict on
the 64 banks, as it did with the old map."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 14
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
    lib.coarse_lds_image_waveload.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.coarse_lds_image_read.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return lib


def _regions(sim):
    r = np.zeros(18, dtype=np.int32)
    sim.coarse_lds_regions(1, r.ctypes.data)
    return {n: (int(r[2 * k]), int(r[2 * k + 1])) for k, n in enumerate(NAMES)}, int(r[14]), int(r[15])


def test_wave_loads_are_consecutive_words(sim):
    image = np.zeros(N, dtype=np.int32)
    sim.coarse_lds_image(image.ctypes.data)
    seen = np.zeros(N, dtype=bool)
    for w in range(16):
        for i in range(16):
            word = np.zeros(64, dtype=np.int32)
            off = np.zeros(64, dtype=np.int32)
            sim.coarse_lds_image_waveload(w, i, word.ctypes.data, off.ctypes.data)
            assert np.array_equal(word, 64 * w + np.arange(64) + 1024 * i)
            assert np.array_equal(off, off[0] + 4 * np.arange(64)), 'wave %d load %d is not lane-linear' % (w, i)
            assert np.array_equal(off, image[word]), 'the load writes where the gather reads'
            assert not seen[word].any()
            seen[word] = True
    assert seen.all(), 'the 256 wave-loads bring every ring word'


def _worst_conflict(sim, old_map):
    worst = 0
    off = np.zeros(64, dtype=np.int32)
    for s0 in range(0, N, 4096):
        for w in range(16):
            for i in range(16):
                sim.coarse_lds_image_read(w, i, s0, old_map, off.ctypes.data)
                assert len(np.unique(off)) == 64
                worst = max(worst, int(np.bincount((off // 4) % 64, minlength=64).max()))
    return worst


def test_bit_reversed_read_within_two_way(sim):
    assert _worst_conflict(sim, 0) <= 2
    # the bound is one the old map (one pad word per 16) meets too
    assert _worst_conflict(sim, 1) <= 2


def test_image_clear_of_ylds_red_and_log_table(sim):
    reg, y_bytes, total = _regions(sim)
    image = np.zeros(N, dtype=np.int32)
    sim.coarse_lds_image(image.ctypes.data)
    off = image.astype(np.int64)
    ybins = np.array([sim.coarse_lds_ybin(q) for q in range(YLEN)], dtype=np.int64)
    assert ybins.max() + 8 == y_bytes
    assert off.min() >= ybins.max() + 8, 'behind every y bin'
    for name in ('red_v', 'red_i', 'logtab'):
        o, s = reg[name]
        assert s > 0
        assert np.all((off + 4 <= o) | (off >= o + s)), 'clear of ' + name
    lo, size = reg['img']
    assert off.min() == lo and off.max() + 4 == lo + size
    two, tws = reg['s_tw']
    assert lo + size <= two or lo + size >= two + tws, 's_tw covered whole or not at all'
    assert total <= 159248, "no more LDS than the image written through registers took"
