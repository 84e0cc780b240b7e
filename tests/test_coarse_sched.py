"""The persistent coarse kernel's channel schedule on the CPU
(aero-cli_amd/csrc/coarse_sched.h, walked by tools/coarse_sched_sim.cpp the
way coarse.hip walks it): a launch of min(nch, G) workgroups, workgroup b
owning channels b, b + grid, ..., scanned 64 at a time with one lane per
channel and a ballot.  Every due channel is visited exactly once, no undue
one is, every channel is scanned exactly once by the workgroup that owns it,
a workgroup visits its channels in rising order, and a channel's state is
preloaded under its predecessor's tail exactly when it is not the first due
channel of its batch."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 64


@pytest.fixture(scope='module')
def sim():
    sys.path.insert(0, os.path.join(ROOT, 'aero-cli_amd'))
    import build
    lib = ctypes.CDLL(build.build_schedsim())
    lib.coarse_sched_sim.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 6
    return lib


def _masks(nch, seed):
    rng = np.random.default_rng(seed)
    yield np.zeros(nch, dtype=np.uint8)
    yield np.ones(nch, dtype=np.uint8)
    for p in (0.02, 0.5, 0.9):
        yield (rng.random(nch) < p).astype(np.uint8)
    one = np.zeros(nch, dtype=np.uint8)  # a workgroup's first channel not due, its last due
    one[nch - 1] = 1
    yield one


@pytest.mark.parametrize('G', [1, 2, 3, 256])
@pytest.mark.parametrize('nch', [1, 2, 5, 70, 257])
def test_every_due_channel_once(sim, G, nch):
    for due in _masks(nch, 1000 * G + nch):
        out = [np.zeros(nch, dtype=np.int32) for _ in range(5)]
        wgs = sim.coarse_sched_sim(nch, G, due.ctypes.data, *[o.ctypes.data for o in out])
        visits, scans, wg_of, seq, pre = out
        assert wgs == min(nch, G)
        assert np.array_equal(visits, due.astype(np.int32)), 'due channels once, undue never'
        assert np.all(scans == 1), 'every channel looked at once'
        assert np.array_equal(wg_of, np.arange(nch) % wgs), 'static stride'
        for wg in range(wgs):
            mine = np.arange(wg, nch, wgs)  # in the order of k
            d = mine[due[mine] == 1]
            assert np.array_equal(seq[d], np.arange(len(d))), 'rising order within a workgroup'
            k = (d - wg) // wgs
            first_of_batch = np.ones(len(d), dtype=bool)
            first_of_batch[1:] = (k[1:] // BATCH) != (k[:-1] // BATCH)
            assert np.array_equal(pre[d], (~first_of_batch).astype(np.int32)), 'preload chain'
        assert np.all(pre[due == 0] == -1)
