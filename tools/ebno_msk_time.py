#!/usr/bin/env python3
"""What AERO_F_EBNO_MSK costs.

One process; per channel count one engine with AERO_F_TIMING | AERO_F_EBNO_MSK
and, with --flag-off, one with AERO_F_TIMING alone: continuous 600-bps MSK
channels at 12 kHz in lockstep, every channel carrying one of a few synthetic
streams; a step pushes one coarse hop (2048 samples) to every channel as one
host batch and runs.  Prints one JSON line per engine: HIP-event milliseconds
per launch of the Eb/N0 kernel beside the demod and coarse kernels of the same
run, the pool's device bytes, and the EbNo of the first channels at the end (so
the run shows what it computed)."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, 'aero-cli_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HOP = 2048
FS = 12000


def leg(ae, pcm, channels, warm, steps, flag=True):
    eng = ae.Engine(max_channels=channels, flags=ae.F_TIMING | (ae.F_EBNO_MSK if flag else 0))
    for _ in range(channels):
        eng.open_channel(600, FS)
    cols = np.arange(channels) % pcm.shape[1]
    for s in range(warm + steps):
        if s == warm:
            eng.sync()
            eng.timing_reset()
        eng.push_batch(pcm[s * HOP:(s + 1) * HOP][:, cols])
        eng.run()
    eng.sync()
    out = {'channels': channels, 'flag': int(flag), 'steps': steps, 'samples_per_step': HOP}
    for k in ('ebno', 'demod', 'coarse', 'frame', 'viterbi'):
        ms, launches = eng.timing('msk600_' + k)
        if launches:
            out[k + '_ms_per_launch'] = round(ms / launches, 4)
            out[k + '_launches'] = launches
    out['ebno_launches_stat'] = eng.stat('ebno_launches')
    out['device_bytes'] = eng.stat('device_bytes')
    out['ebno_first'] = [round(eng.channel_quality(c)['ebno_db'], 3) for c in range(min(4, channels))]
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--channels', default='64,4096')
    ap.add_argument('--warmup', type=int, default=4, help='untimed steps of one hop')
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--pool', type=int, default=8, help='distinct synthetic streams')
    ap.add_argument('--flag-off', action='store_true', help='also a leg without AERO_F_EBNO_MSK per channel count')
    a = ap.parse_args()
    import aero_engine as ae
    import aero_testlib as tl
    n = (a.warmup + a.steps) * HOP
    pcm = np.stack([tl.synth_msk(seconds=n / FS + 0.01, bitrate=600, seed=0xEB40 + k, carrier=600.0 + 40 * k, fs=FS)[:n]
                    for k in range(a.pool)], axis=1)
    for ch in [int(c) for c in a.channels.split(',')]:
        for flag in ((True, False) if a.flag_off else (True,)):
            print(json.dumps(leg(ae, pcm, ch, a.warmup, a.steps, flag)), flush=True)


if __name__ == '__main__':
    main()
