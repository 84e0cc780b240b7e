#!/usr/bin/env python3
"""What AERO_F_DCD_TICK_CONT costs.

One process, one many-channel workload per kind (msk600 at 12 kHz, msk1200 at
24 kHz, c8400), three engines one after the other with AERO_F_TIMING: the flag
off, on, and off again.  Every channel carries one of a few synthetic streams;
a step pushes half a second to every channel (one host batch) and runs.  Prints
one JSON line per leg: wall and per-kernel HIP-event milliseconds per timed
step, the host frame section, and the DCD edges of the first 64 channels
(which only the flag moves)."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'aero-cli_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

KINDS = {'msk600': (600, 12000, 'msk600_'), 'msk1200': (1200, 24000, 'msk1200_'), 'c8400': (8400, 48000, 'c8400_')}
KERNELS = ('coarse', 'prefilter', 'demod', 'frame', 'viterbi', 'host_frames', 'host_run')


def streams(kind, seconds, pool):
    import aero_testlib as tl
    bitrate, fs, _ = KINDS[kind]
    if kind == 'c8400':
        return [tl.synth_c(seconds=seconds, seed=0xC700 + k, carrier=11000.0 + 50 * k) for k in range(pool)]
    return [tl.synth_msk(seconds=seconds, bitrate=bitrate, baud=600, seed=0xC600 + k, carrier=600.0 + 20 * k,
                         ebn0=14.0, fs=fs) for k in range(pool)]


def leg(ae, kind, flag, pcm, channels, warm, steps):
    bitrate, fs, tag = KINDS[kind]
    eng = ae.Engine(max_channels=channels, flags=ae.F_TIMING | (ae.F_DCD_TICK_CONT if flag else 0))
    for _ in range(channels):
        eng.open_channel(bitrate, fs)
    n = fs // 2
    cols = np.arange(channels) % len(pcm)
    wall = 0.0
    for s in range(warm + steps):
        if s == warm:
            eng.sync()
            eng.timing_reset()
        x = np.stack([p[s * n:(s + 1) * n] for p in pcm], axis=1)[:, cols]
        t0 = time.perf_counter()
        eng.push_batch(x)
        eng.run()
        if s >= warm:
            eng.sync()
            wall += time.perf_counter() - t0
    eng.flush()
    out = {'kind': kind, 'flag': int(flag), 'channels': channels, 'steps': steps,
           'library': os.environ.get('AERO_ENGINE_SO', 'libaero_engine.so'),
           'ms_per_step': round(wall * 1e3 / steps, 3)}
    for k in KERNELS:
        ms, launches = eng.timing(k if k.startswith('host_') else tag + k)
        if launches:
            out[k] = round(ms / steps, 4)
    out['edges_first_64'] = sum(eng.channel_events(c)[0] for c in range(min(64, channels)))
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--kinds', default='msk600,msk1200,c8400')
    ap.add_argument('--channels', type=int, default=8192)
    ap.add_argument('--warmup', type=int, default=12, help='untimed steps of half a second (the channels lock)')
    ap.add_argument('--steps', type=int, default=12)
    a = ap.parse_args()
    import aero_engine as ae
    for kind in a.kinds.split(','):
        ch = a.channels // 4 if kind == 'c8400' else a.channels
        pcm = streams(kind, (a.warmup + a.steps) / 2.0, 8)
        for flag in (False, True, False):
            print(json.dumps(leg(ae, kind, flag, pcm, ch, a.warmup, a.steps)), flush=True)


if __name__ == '__main__':
    main()
