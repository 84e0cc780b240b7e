"""bench.ItemTap.arrays (--dump-outputs) on hand-made item records: per
channel the last items in delivery order whatever drain delivered them,
counts over the whole region, bytes past the lengths zeroed."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _record(ae, width, aes, msg, junk):
    it = ae.AcarsItem()
    ctypes.memset(ctypes.addressof(it), junk, ctypes.sizeof(it))  # what the engine leaves past the lengths
    it.aesid, it.label_len, it.reg_len, it.msg_len = aes, 2, 3, len(msg)
    ctypes.memmove(ctypes.addressof(it) + ae.AcarsItem.msg.offset, msg, len(msg))
    return np.frombuffer(bytes(it), dtype=np.uint8)[:width].copy()


def _tap(drains):
    import bench
    import aero_engine as ae
    tap = bench.ItemTap(None, 16)
    for d in drains:
        ch = np.array([c for c, _, _ in d], dtype=np.int32)
        tap.kept.append((ch, np.stack([_record(ae, tap.width, aes, msg, 0xEE) for _, aes, msg in d])))
    return tap, ae


def test_arrays_order_counts_and_masking():
    import bench
    seq = [(3, 100 + i, b'm%02d' % i) for i in range(11)]  # channel 3: eleven items, more than are kept
    one = [(5, 7, b'x' * 300)]                              # channel 5: one item, longer than DUMP_MSG
    whole, ae = _tap([seq[:4] + one, seq[4:]])
    split, _ = _tap([seq[:9], one + seq[9:]])               # the same items delivered by other drains
    a, b = whole.arrays(), split.arrays()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    I = ae.AcarsItem
    assert np.array_equal(a['acars_channels'], np.arange(16))
    assert a['acars_item_counts'][3] == 11 and a['acars_item_counts'][5] == 1 and a['acars_item_counts'].sum() == 12
    items = a['acars_items']
    assert items.shape == (16, bench.DUMP_LAST, I.msg.offset + bench.DUMP_MSG) and items.dtype == np.float32
    # channel 3: its last eight, oldest first
    assert items[3, :, 0].tolist() == [100 + i for i in range(3, 11)]
    assert bytes(items[3, -1, I.msg.offset:I.msg.offset + 3].astype(np.uint8)) == b'm10'
    assert not items[3, :, I.msg.offset + 3:].any()                      # past msg_len
    assert (items[3, :, I.label.offset:I.label.offset + 2] == 0xEE).all()
    assert not items[3, :, I.label.offset + 2:I.label.offset + I.label.size].any()
    assert not items[3, :, I.reg.offset + 3:I.reg.offset + I.reg.size].any()
    # channel 5: one item in the last row, its message cut at DUMP_MSG bytes, msg_len kept
    assert not items[5, :-1].any()
    assert (items[5, -1, I.msg.offset:] == ord('x')).all()
    assert items[5, -1, I.msg_len.offset] + 256 * items[5, -1, I.msg_len.offset + 1] == 300
    assert not items[[c for c in range(16) if c not in (3, 5)]].any()
