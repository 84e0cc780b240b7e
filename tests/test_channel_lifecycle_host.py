"""Channel lifecycle, the parts that need no GPU.

aero_channel_close / aero_engine_reserve refuse a null engine, and the reset
plan (csrc/slot_reset.h): the byte ranges the reset kernel writes for a closed
channel's slot, as layout() / burst_layout() record them.  An index slip in
that table is an out-of-bounds device write, so the addressing is pinned here:
every range inside the pool, none in a table or a group-wide array, the
ranges of two slots disjoint, and for a 64-channel pool every byte of every
per-channel array written by exactly one slot."""
import ctypes

import numpy as np
import pytest

# aero_x_reset_plan kinds: a Mode, a generic-rate MSK Mode | fs << 8, 100 + BurstKind
MODE_MSKG600, MODE_C8400 = 8, 10
KINDS = {
    'oqpsk': 0, 'msk600': 1, 'msk1200': 2, 'msk600_24k': 3, 'msk600_48k': 4, 'msk1200_12k': 5, 'msk1200_48k': 6,
    'mskg600_18750': MODE_MSKG600 | (18750 << 8),  # SPS 31
    'c8400': MODE_C8400, 'burst_oqpsk': 100, 'burst_msk': 101,
}
F_TRACE_PT, F_TRACE_BLOCKS, F_TRACE_SOFT, F_TRACE_HOPS, F_DCD_TICK = 1, 2, 4, 8, 64
TRACE = F_TRACE_PT | F_TRACE_BLOCKS | F_TRACE_SOFT | F_TRACE_HOPS
RS_SHARED, RS_COL, RS_ROW, RS_END = 0, 1, 2, 3


def _plan(L, kind, C, flags, slot):
    n = L.aero_x_reset_plan(kind, C, flags, slot, None, 0)
    assert n > 0, 'aero_x_reset_plan(%d, %d, %d, %d) = %d' % (kind, C, flags, slot, n)
    out = np.zeros((n, 7), dtype=np.uint64)
    assert L.aero_x_reset_plan(kind, C, flags, slot, out.ctypes.data_as(ctypes.c_void_p), n) == n
    return [tuple(int(v) for v in r) for r in out]


def _ranges(plan):
    """starts and ends (arrays) of every row of every entry of one slot's plan"""
    st, en = [], []
    for start, elem, rows, pitch, kind, fill, total in plan:
        assert kind in (RS_COL, RS_ROW) and elem > 0 and rows > 0
        assert rows == 1 or pitch >= elem
        a = start + np.arange(rows, dtype=np.int64) * pitch
        st.append(a)
        en.append(a + elem)
    return np.concatenate(st), np.concatenate(en)


def _add(hits, plan):
    """hits[byte] += 1 for every byte of one slot's plan"""
    for start, elem, rows, pitch, kind, fill, total in plan:
        assert 0 <= start and start + (rows - 1) * pitch + elem <= len(hits)
        v = np.lib.stride_tricks.as_strided(hits[start:], shape=(rows, elem), strides=(max(pitch, elem), 1))
        v += 1


def _layout(L, kind, C, flags):
    """pool size, extents of the per-channel arrays, extents of everything else"""
    arrays = _plan(L, kind, C, flags, -1)
    assert arrays[-1][4] == RS_END
    pool = arrays[-1][0]
    per = [(a[0], a[0] + a[6]) for a in arrays[:-1] if a[4] != RS_SHARED]
    shared = [(a[0], a[0] + a[6]) for a in arrays[:-1] if a[4] == RS_SHARED]
    ext = sorted(per + shared)
    assert all(x[1] <= y[0] for x, y in zip(ext, ext[1:])) and ext[-1][1] <= pool, 'arrays overlap'
    return pool, per, shared


def test_null_engine_is_invalid(engine_lib):
    import aero_engine as ae
    assert engine_lib.aero_channel_close(None, 0) == ae.AERO_E_INVALID
    cfg = ae.ChannelCfg(8400, 0, 48000, 0)
    assert engine_lib.aero_engine_reserve(None, ctypes.byref(cfg), 4) == ae.AERO_E_INVALID


def test_reset_plan_arguments(engine_lib):
    L = engine_lib
    for kind, C, slot in ((0, 63, 0), (0, 64, 64), (0, 64, -2), (7, 64, 0), (102, 64, 0), (1 | (12000 << 8), 64, 0)):
        assert L.aero_x_reset_plan(kind, C, 0, slot, None, 0) < 0, (kind, C, slot)


def test_shared_arrays_are_the_expected_ones(engine_lib):
    """What the layouts mark as no slot's: the tables, the job lists and
    counters, and the placeholders of arrays a mode does not use."""
    for name, flags in (('oqpsk', TRACE), ('c8400', TRACE)):
        arrays = _plan(engine_lib, KINDS[name], 64, flags, -1)[:-1]
        # jobs, njobs, jobout + 11 tables, and the one-element placeholders
        # (OQPSK: dsm, d8, ms, cin, cout, csig, crem; C: dsm, d8, ms)
        assert sum(a[4] == RS_SHARED for a in arrays) == 14 + (7 if name == 'oqpsk' else 3), name
    for name in ('burst_oqpsk', 'burst_msk'):
        arrays = _plan(engine_lib, KINDS[name], 64, 0, -1)[:-1]
        # tjobs, ntjobs, jobs, njobs, jobout, tri_abs + 9 tables + 3 x 7 delay tables
        assert sum(a[4] == RS_SHARED for a in arrays) == 6 + 9 + 21, name


@pytest.mark.parametrize('flags', [0, TRACE, F_DCD_TICK], ids=['plain', 'trace', 'dcd'])
@pytest.mark.parametrize('C', [64, 128, 4096])
@pytest.mark.parametrize('name', sorted(KINDS))
def test_reset_plan_stays_in_its_slot(engine_lib, name, C, flags):
    L = engine_lib
    kind = KINDS[name]
    pool, per, shared = _layout(L, kind, C, flags)
    lo = np.array([x[0] for x in sorted(per)], dtype=np.int64)
    hi = np.array([x[1] for x in sorted(per)], dtype=np.int64)
    slots = [0, 1, C - 1]
    rng = {s: _ranges(_plan(L, kind, C, flags, s)) for s in slots}
    for s in slots:
        a, b = rng[s]
        assert np.all((0 <= a) & (a < b) & (b <= pool)), 'slot %d writes outside the pool of %d bytes' % (s, pool)
        # every range inside one per-channel array (the arrays are disjoint:
        # _layout), so in no table and no group-wide array
        k = np.searchsorted(lo, a, side='right') - 1
        assert np.all(k >= 0) and np.all(b <= hi[np.maximum(k, 0)]), 'slot %d writes outside its arrays' % s
    # two slots never share a byte: sort every range and look at neighbours
    a = np.concatenate([rng[s][0] for s in slots])
    b = np.concatenate([rng[s][1] for s in slots])
    o = np.argsort(a, kind='stable')
    assert np.all(b[o][:-1] <= a[o][1:]), 'two slots overlap'
    # the same entries, the same bytes per slot
    assert len({len(rng[s][0]) for s in slots}) == 1
    assert len({int(np.sum(rng[s][1] - rng[s][0])) for s in slots}) == 1


@pytest.mark.parametrize('flags', [0, TRACE], ids=['plain', 'trace'])
@pytest.mark.parametrize('name', sorted(KINDS))
def test_reset_plan_covers_every_channel_byte_once(engine_lib, name, flags):
    """C = 64: the 64 slots' ranges together are the per-channel arrays
    exactly, each byte written by one slot."""
    L = engine_lib
    kind, C = KINDS[name], 64
    pool, per, shared = _layout(L, kind, C, flags)
    hits = np.zeros(pool, dtype=np.uint8)
    for s in range(C):
        _add(hits, _plan(L, kind, C, flags, s))
    want = np.zeros(pool, dtype=np.uint8)
    for a, b in per:
        want[a:b] += 1
    assert want.max() == 1
    assert np.array_equal(hits, want), '%d bytes reset twice or not at all' % int(np.count_nonzero(hits != want))
    # scalar fields carry their initial values: ds rows doubles, is rows ints
    fills = {(p[1], p[5]) for p in _plan(L, kind, C, flags, 0)}
    assert (8, 1) in fills and (4, 2) in fills
