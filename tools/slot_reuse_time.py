#!/usr/bin/env python3
"""What reusing a channel slot costs.

Default: the one reuse every build of the engine has.  A 600-bps MSK channel
leaves the 12 kHz group for another rate (its slot becomes free), then a new
600-bps channel opened at 12 kHz takes that slot.  Timed: that open plus the
next run() + sync(), on a fresh engine per repeat; prints the median and the
spread (max - min) of the repeats as one JSON line.  Uses only
open_channel / push / run / sync, so a build from before aero_channel_close
runs it unchanged (AERO_ENGINE_SO selects the library).

--batch N: closes and reopens N of --channels OQPSK channels in one batch and
times close + reopen + run() + sync() (needs aero_channel_close)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'aero-cli_amd'))


def single(ae, repeats):
    rng = np.random.default_rng(7)
    audio = (rng.standard_normal(24000) * 3000).astype(np.int16)  # 2 s at 12 kHz: the slot carries state
    out = []
    for _ in range(repeats):
        eng = ae.Engine(max_channels=64)
        a = eng.open_channel(600, 12000)
        b = eng.open_channel(600, 12000)
        for ch in (a, b):
            eng.push(ch, audio, fs=12000)
        eng.run()
        eng.sync()
        eng.push(a, audio[:64], fs=24000)  # a moves to the 24 kHz group; its 12 kHz slot is free
        t0 = time.perf_counter()
        eng.open_channel(600, 12000)
        eng.run()
        eng.sync()
        out.append((time.perf_counter() - t0) * 1e3)
        eng.close()
    return out


def batch(ae, repeats, channels, n):
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((12000, channels)) * 3000).astype(np.int16)
    out = []
    for _ in range(repeats):
        eng = ae.Engine(max_channels=channels)
        chans = [eng.open_channel(10500, 48000) for _ in range(channels)]
        eng.push_batch(x)
        eng.run()
        eng.sync()
        victims = chans[::channels // n][:n]
        t0 = time.perf_counter()
        for ch in victims:
            eng.close_channel(ch)
        for _ in victims:
            eng.open_channel(10500, 48000)
        eng.run()
        eng.sync()
        out.append((time.perf_counter() - t0) * 1e3)
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--batch', type=int, default=0, help='close and reopen this many OQPSK channels in one batch')
    ap.add_argument('--channels', type=int, default=4096)
    a = ap.parse_args()
    import aero_engine as ae
    ms = batch(ae, a.repeats, a.channels, a.batch) if a.batch else single(ae, a.repeats)
    print(json.dumps({'scenario': 'batch_%d_of_%d' % (a.batch, a.channels) if a.batch else 'msk_slot_reuse',
                      'library': os.environ.get('AERO_ENGINE_SO', 'libaero_engine.so'),
                      'ms': [round(v, 3) for v in ms], 'median_ms': round(statistics.median(ms), 3),
                      'spread_ms': round(max(ms) - min(ms), 3)}))


if __name__ == '__main__':
    main()
