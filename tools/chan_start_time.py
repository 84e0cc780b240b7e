"""Start latency of a batch of 64 VFOs: aero_chan_vfo_open x 64 + the start
kernel (device NCO fill), against the same 64 tables from host_pub_osc copied
to the device (what create did before), pageable and through pinned staging."""
import ctypes
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

cfg = tl.c5_config()
lib = ae.load_library()
res = {}

ch = ae.Channeliser(cfg['sample_rate'], cfg['center_frequency'], cfg['mains'], [], max_blocks=1)
shapes = {}
for d in cfg['vfos']:
    main = min(range(3), key=lambda m: abs(d['frequency'] - cfg['mains'][m]['frequency']))
    shapes.setdefault((main, d['data_rate'], d.get('filter_bandwidth', 0)), []).append(d)
for ds in shapes.values():
    ch.reserve(ds[0], len(ds))
assert ch.stat('slots_free') == 64
ch.run()
ch.sync()
dev, opens = [], []
for rep in range(5):
    nbytes, inits = ch.stat('device_bytes'), ch.stat('vfo_inits')
    t0 = time.perf_counter()
    ids = [ch.open_vfo(d) for d in cfg['vfos']]
    t1 = time.perf_counter()
    ch.run()  # nothing pending: launches the start kernel
    ch.sync()
    t2 = time.perf_counter()
    assert ch.stat('device_bytes') == nbytes and ch.stat('vfo_inits') == inits + 1
    dev.append((t2 - t0) * 1e3)
    opens.append((t1 - t0) * 1e3)
    for v in ids:
        ch.close_vfo(v)
res['device_fill_ms'] = dev
res['of_which_open_calls_ms'] = opens
ch.close()

fs = 192000
freqs = [float((i * 2500) % 90000 - 45000) for i in range(64)]
dst = torch.empty((64, fs * 2), dtype=torch.float32, device='cuda')
torch.cuda.synchronize()
host = []
for rep in range(5):
    t0 = time.perf_counter()
    for i, f in enumerate(freqs):
        a = np.empty(fs * 2, dtype=np.float32)
        lib.aero_host_pub_osc(ctypes.c_double(fs), ctypes.c_double(f), a.ctypes.data_as(ctypes.c_void_p))
        dst[i].copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    host.append((time.perf_counter() - t0) * 1e3)
res['host_fill_pageable_copy_ms'] = host

pin = torch.empty((64, fs * 2), dtype=torch.float32).pin_memory()
pinned = []
for rep in range(5):
    t0 = time.perf_counter()
    for i, f in enumerate(freqs):
        lib.aero_host_pub_osc(ctypes.c_double(fs), ctypes.c_double(f), ctypes.c_void_p(pin[i].data_ptr()))
        dst[i].copy_(pin[i], non_blocking=True)
    torch.cuda.synchronize()
    pinned.append((time.perf_counter() - t0) * 1e3)
res['host_fill_pinned_copy_ms'] = pinned

print(json.dumps({k: [round(x, 3) for x in v] for k, v in res.items()}))
