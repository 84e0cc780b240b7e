"""Shared by tests/test_chan_start_model.py and tests/test_gpu_chan_lifecycle.py:
the settle bound of a [vfos] entry from the oracle's own figures, and the
oracle channeliser's outputs per (configuration, reads, input variant),
computed once and handed out read-only."""
import functools
import math

import numpy as np

import aero_testlib as tl

C = tl.CENTER
SEED = 7


def main_stages(cfg, m):
    r = cfg['sample_rate'] // cfg['mains'][m]['out_rate']
    return 0 if r == 1 else int(math.log2(r))


def bound(cfg, info):
    """124 + usb_taps + ceil(late_taps / late) + 12 * (stages + main stages), from oracle_pub_info."""
    b = 124 + info['usb_taps'] + 12 * (info['halfbands'] + main_stages(cfg, info['main']))
    if info['late']:
        b += -(-info['late_taps'] // info['late'])
    return b


def config(name):
    if name == 'c5':
        return dict(tl.c5_config(), tones=[])
    return tl.PUB_CONFIGS[name]


@functools.lru_cache(maxsize=None)
def block_len(name):
    cfg = config(name)
    return tl.OraclePublisher(cfg['sample_rate'], C, cfg['mains'], cfg['vfos']).block_len


@functools.lru_cache(maxsize=None)
def wideband(name, nreads, silent=(0, 0)):
    """nreads reads of the configuration's test input; reads silent[0] .. silent[1]-1 zeroed."""
    cfg = config(name)
    x = tl.wideband(cfg['sample_rate'], nreads * block_len(name), SEED, cfg['tones'])
    x[silent[0] * block_len(name):silent[1] * block_len(name)] = 0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def oracle(name, nreads, silent=(0, 0)):
    """(infos, [audio of every VFO], [IQ of every main]) of the always-present oracle."""
    cfg = config(name)
    ref = tl.OraclePublisher(cfg['sample_rate'], C, cfg['mains'], cfg['vfos'])
    ref.process(wideband(name, nreads, silent))
    infos = [ref.info(v) for v in range(len(cfg['vfos']))]
    usb = [ref.usb(v) for v in range(len(cfg['vfos']))]
    iq = [ref.iq(m) for m in range(len(cfg['mains']))]
    for a in usb + iq:
        a.setflags(write=False)
    return infos, usb, iq
