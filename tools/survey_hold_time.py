"""What the survey's peak / min hold costs: tools/survey_time.py's
measurement (wall time of 64 reads through aero_chan_push (device pointer) +
aero_chan_run, then aero_chan_sync, one read per run, at 288 ksps and
1.92 Msps) with the survey off, on at log2n 12 and 14, the same with a hold of
groups of 4 segments without a ring, the same with a ring of 64 rows, and off
again.  One JSON line per case: milliseconds per read of three repetitions,
launches per read and device_bytes."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'aero-cli_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import aero_engine as ae  # noqa: E402
import aero_testlib as tl  # noqa: E402

READS, POOL, REPS = 64, 8, 3
GROUP = 4
# (survey_log2n, hold rows; None: no hold)
CASES = [(0, None), (12, None), (14, None), (12, 0), (14, 0), (12, 64), (14, 64), (0, None)]

for name in ('r288k', 'r1920k'):
    cfg = tl.PUB_CONFIGS[name]
    fs = cfg['sample_rate']
    ch = ae.Channeliser(fs, tl.CENTER, cfg['mains'], cfg['vfos'], max_blocks=1)
    B = ch.block_len
    x = tl.wideband(fs, POOL * B, 0x7E, cfg['tones'])
    dev = torch.from_numpy(x.view(np.float32)).to('cuda')
    torch.cuda.synchronize()

    def reads(n):
        for r in range(n):
            ch.push_device(dev.data_ptr() + (r % POOL) * B * 8, 1)
            ch.run()
        ch.sync()

    for log2n, rows in CASES:
        if log2n:
            ch.survey_start(log2n, 'hann')
        if rows is not None:
            ch.survey_hold_start(GROUP, rows)
        reads(POOL)  # warm-up
        launches, groups0 = ch.stat('survey_launches'), ch.stat('survey_groups')
        ms = []
        for rep in range(REPS):
            t0 = time.perf_counter()
            reads(READS)
            ms.append((time.perf_counter() - t0) * 1e3 / READS)
        segs, nbytes = 0, ch.stat('device_bytes')
        if log2n:
            segs = ch.survey_read()[1]
            ch.survey_stop()  # ends the hold
        print(json.dumps(dict(config=name, sample_rate=fs, read_ms=round(1e3 * B / fs, 3), survey_log2n=log2n,
                              hold_group=GROUP if rows is not None else 0, hold_rows=rows or 0,
                              ms_per_read=[round(v, 4) for v in ms], segments=segs,
                              groups=ch.stat('survey_groups') - groups0,
                              launches_per_read=(ch.stat('survey_launches') - launches) / (REPS * READS),
                              device_bytes=nbytes)), flush=True)
    ch.close()
