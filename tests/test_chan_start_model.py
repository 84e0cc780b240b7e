"""The model behind the channeliser's run-time VFOs (include/aero_chan.h,
DESIGN.md §3b), on the CPU.

Every stage of a VFO has finite memory and the NCO is a table indexed by the
sample count, so the oracle channeliser (oracle/pub_oracle.cpp) fed x and the
oracle fed x with its first k reads zeroed agree on every VFO from sample
k*S + bound on, with bound = 124 + usb_taps + ceil(late_taps/late) +
12*(stages + main stages) below one read.  The second oracle is what a VFO
opened at read k with zero histories computes (tests/test_gpu_chan_lifecycle.py
holds the GPU to it), so this pins the settle bound the GPU tests rely on.

Then the host bookkeeping of chan.hip (aero-cli_amd/csrc/chan_slots.h through
tools/chan_slots_sim.cpp): the id allocator, the free lists of slots per
shape and the settle formula."""
import ctypes
import os
import sys

import numpy as np
import pytest

import chan_start_lib as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def sim(cpu_libs):
    sys.path.insert(0, os.path.join(ROOT, 'aero-cli_amd'))
    import build
    lib = ctypes.CDLL(build.build_chanslots())
    lib.chan_ids_sim.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.chan_pool_sim.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.chan_settle_sim.argtypes = [ctypes.c_int] * 5
    lib.chan_settle_sim.restype = ctypes.c_longlong
    return lib


@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('name', ['r1536k', 'r288k', 'r1920k'])
def test_late_start_agrees_after_bound(cpu_libs, sim, name, k):
    cfg = cs.config(name)
    n = k + 2
    infos, full, _ = cs.oracle(name, n)
    _, late, _ = cs.oracle(name, n, silent=(0, k))
    for v, info in enumerate(infos):
        S, b = info['samples_per_block'], cs.bound(cfg, info)
        assert b < S, 'the settle bound is below one read'
        assert len(full[v]) == len(late[v]) == n * S
        assert not late[v][:k * S].any(), 'silent input, silent audio'
        diff = np.flatnonzero(full[v] != late[v])
        print('%s vfo %d k %d: last differing sample %d after read k, bound %d' % (
            name, v, k, (diff.max() - k * S) if diff.size else -1, b))
        assert np.array_equal(full[v][k * S + b:], late[v][k * S + b:])
        assert np.count_nonzero(full[v][k * S + b:]) > (len(full[v]) - k * S - b) // 2
        got = sim.chan_settle_sim(info['usb_taps'], info['late_taps'], info['late'], info['halfbands'],
                                  cs.main_stages(cfg, info['main']))
        assert 124 <= got <= b


def test_settle_formula(sim):
    assert sim.chan_settle_sim(0, 0, 0, 0, 0) == 124  # the Hilbert transformer alone
    assert sim.chan_settle_sim(77, 0, 0, 2, 3) == 124 + 77 + 12 * 5
    assert sim.chan_settle_sim(0, 63, 5, 1, 0) == 124 + 13 + 12  # ceil(63 / 5)
    assert sim.chan_settle_sim(0, 60, 6, 0, 0) == 124 + 10


def _ids(sim, ops):
    ops = np.asarray(ops, dtype=np.int32)
    out, cnt = np.zeros(len(ops), np.int32), np.zeros(len(ops), np.int32)
    sim.chan_ids_sim(ops.ctypes.data, len(ops), out.ctypes.data, cnt.ctypes.data)
    return out.tolist(), cnt.tolist()


def test_ids_smallest_free_first(sim):
    T = -1
    out, cnt = _ids(sim, [T, T, T, T, 1, 2, T, T, T, 4, 0, T])
    #                     0  1  2  3  r1 r2 1  2  4  r4 r0 0
    assert out == [0, 1, 2, 3, 1, 1, 1, 2, 4, 1, 1, 0]
    assert cnt == [1, 2, 3, 4, 4, 4, 4, 4, 5, 4, 4, 4]


def test_ids_release_errors_and_count(sim):
    T = -1
    out, cnt = _ids(sim, [5, T, 0, 0, T, T, T, 2, 1, 1, 7, T])
    # release of an id never given out, a double release, one past the end: refused
    assert out == [0, 0, 1, 0, 0, 1, 2, 1, 1, 0, 0, 1]
    # the count is one past the largest id in use, and falls when that one goes
    assert cnt == [0, 1, 0, 0, 1, 2, 3, 2, 1, 1, 1, 2]


def test_ids_against_a_model(sim):
    rng = np.random.default_rng(5)
    used, ops, want, wcnt = set(), [], [], []
    for _ in range(400):
        if used and rng.random() < 0.45:
            i = int(rng.integers(0, max(used) + 2))
            ops.append(i)
            want.append(int(i in used))
            used.discard(i)
        else:
            i = next(j for j in range(len(used) + 1) if j not in used)
            ops.append(-1)
            want.append(i)
            used.add(i)
        wcnt.append(max(used) + 1 if used else 0)
    out, cnt = _ids(sim, ops)
    assert out == want and cnt == wcnt


def _pool(sim, ops):
    ops = np.asarray(ops, dtype=np.int32).reshape(-1, 9)
    out, nfree = np.zeros(len(ops), np.int32), np.zeros(len(ops), np.int32)
    sim.chan_pool_sim(ops.ctypes.data, len(ops), out.ctypes.data, nfree.ctypes.data)
    return out.tolist(), nfree.tolist()


def test_slot_pool_per_shape_smallest_first(sim):
    A = [0, 2, 0, 48000, 12000, 48000, 0]
    PUT, TAKE = 0, 1
    ops = [[PUT, 5] + A, [PUT, 3] + A, [PUT, 9] + A]
    # every field is part of the shape: a slot of A serves none of these
    others = [A[:i] + [A[i] + 1] + A[i + 1:] for i in range(7)]
    ops += [[TAKE, 0] + o for o in others]
    ops += [[PUT, 4] + others[6], [TAKE, 0] + A, [TAKE, 0] + others[6], [TAKE, 0] + others[6], [TAKE, 0] + A,
            [PUT, 3] + A, [TAKE, 0] + A, [TAKE, 0] + A, [TAKE, 0] + A]
    out, nfree = _pool(sim, ops)
    assert out == [0, 0, 0] + [-1] * 7 + [0, 3, 4, -1, 5, 0, 3, 9, -1]
    assert nfree == [1, 2, 3] + [3] * 7 + [4, 3, 2, 2, 1, 2, 1, 0, 0]
