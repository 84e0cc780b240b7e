"""bench.py's plain run and --dump-outputs on a small batch: the plain line
carries the headline fields and none of the --full measurements, and the
dump is the timed region's ACARS items (bench.ItemTap) as float .npy files
that agree with the line's own counters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, STEPS = 64, 6


def test_plain_run_and_dump(tmp_path):
    out_dir = tmp_path / 'dump'
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(STEPS),
                        '--warmup', '1', '--channels', str(C), '--dump-outputs', str(out_dir)],
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout[-3000:]
    out = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in out
    assert out['steps'] == STEPS and out['ms_per_step'] > 0
    # one step is one hop of every channel
    assert out['value'] == pytest.approx(C * 4096 / (out['ms_per_step'] * 1e3), rel=1e-3)
    assert 'cpu_baseline' not in out and 'vs_cpu' not in out and 'h2d' not in out

    arrays = {f[:-4]: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}
    assert sorted(arrays) == ['acars_channels', 'acars_item_counts', 'acars_items', 'timed_region']
    assert all(v.dtype in (np.float32, np.float64) for v in arrays.values())
    assert sum(v.nbytes for v in arrays.values()) <= 64 << 20
    # fewer channels than the sample holds: every channel is in it
    assert np.array_equal(arrays['acars_channels'], np.arange(C))
    tr = out['timed_region']
    assert arrays['timed_region'].tolist() == [STEPS * C * 4096] + [tr[k] for k in sorted(tr)]
    counts, items = arrays['acars_item_counts'], arrays['acars_items']
    assert counts.sum() == tr['acars_items'] > 0
    assert items.shape[:2] == (C, 8)
    # a channel's kept items fill the rows at the end (no item record is all zero: its AES id is not)
    filled = (items != 0).any(axis=2)
    assert np.array_equal(filled.sum(axis=1), np.minimum(counts, 8))
    assert filled[counts > 0, -1].all()
