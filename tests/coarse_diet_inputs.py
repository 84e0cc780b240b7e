"""Inputs of the coarse kernel's log10 / mix tests (tests/test_math_log10_ge1.py,
tests/test_coarse_near1_inputs.py on the CPU; tests/test_gpu_coarse_diet.py on
the GPU).

log10's argument in the coarse estimator is max(|X|, 1).  aero_log10_ge1_tab
(aero_math.h) splits it into exponent and mantissa m in [1, 2); log takes its
polynomial around 1 for m < NEAR_HI and its table otherwise, lane by lane.
near1() is that test, on |X| as the oracle reports it."""
import ctypes
import functools

import numpy as np

import aero_testlib as tl  # noqa: F401  (puts the package on sys.path)
import coarse_inputs as ci
import mathhost

HOST_LOG10_GE1 = 15  # tools/mathhost.cpp
NEAR_HI = 0x3ff1090000000000  # 1 + 0x1.09p-4: log's near-1 bound (e_log.c HI)


def host_log10_ge1(x):
    """aero_log10_ge1 as the host compiles it (finite x >= 1)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.zeros_like(x)
    out = np.empty_like(x)
    mathhost.lib().aero_math_host_eval(HOST_LOG10_GE1, ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(y.ctypes.data),
                                       ctypes.c_void_p(out.ctypes.data), x.size)
    return out


def boundary_set():
    """1.0; the near-1 bound and both its neighbours in every binade; 2^k and
    its neighbours for k = 0 ... 1023 (not the one below 1); DBL_MAX."""
    e = np.arange(1024, dtype=np.uint64) << np.uint64(52)
    bound = np.uint64(NEAR_HI) + e
    pow2 = np.uint64(0x3ff0000000000000) + e
    bits = np.concatenate([bound - np.uint64(1), bound, bound + np.uint64(1), pow2, pow2 + np.uint64(1),
                           pow2[1:] - np.uint64(1), np.array([0x7fefffffffffffff], dtype=np.uint64)])
    x = bits.view(np.float64)
    assert np.isfinite(x).all() and (x >= 1.0).all() and x[0] < x[1024] and x.max() == np.finfo(np.float64).max
    return x


def near1(absx):
    """Which bins take log's near-1 polynomial: the mantissa of max(|X|, 1) below NEAR_HI."""
    a = np.maximum(np.ascontiguousarray(absx, dtype=np.float64), 1.0)
    m = (a.view(np.uint64) & np.uint64(0x000fffffffffffff)) | np.uint64(0x3ff0000000000000)
    return m < np.uint64(NEAR_HI)


# The GPU test's modes, and per mode two engines of three channels.  Streams:
#   silence_carrier  coarse_inputs': silence until the hunter steps, then a
#                    carrier 40 Hz off the new centre (the AFC retunes: yreset)
#   lsb_noise        coarse_inputs': +-1 LSB, |X| on both sides of 1
#   hunting          a carrier the estimator's first centre does not reach:
#                    AFC retunes and hunter steps (zero_before inside the snapshot)
#   locked           a carrier the AFC pulls in within a few hops, then steady
MODES = ('oqpsk10500@48000', 'c8400@48000', 'msk600@12000')
TRIOS = {'a': ('silence_carrier', 'lsb_noise', 'hunting'), 'b': ('locked', 'hunting', 'silence_carrier')}
SEED = 0xD1E7
# carrier and hops of 'hunting' / 'locked' (the MSK estimator works at 12 kHz)
CARRIERS = {
    'oqpsk10500@48000': {'hunting': (20000.0, 64), 'locked': (12037.5, 40)},
    'c8400@48000': {'hunting': (20000.0, 64), 'locked': (12037.5, 40)},
    'msk600@12000': {'hunting': (2500.0, 64), 'locked': (1010.0, 40)},
}


@functools.lru_cache(maxsize=None)
def stream(mode, name):
    hop = ci.MODES[mode][2]
    if name in ('silence_carrier', 'lsb_noise'):
        return dict(ci.streams(mode))[name]
    f, hops = CARRIERS[mode][name]
    x = ci._carrier(mode, f, hops * hop + ci.TAIL, SEED + (1 if name == 'locked' else 0))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def walk(mode, name):
    """The oracle over one stream, one hop per message: per hop (|X| of the kept
    bins, y of the kept bins, hop records so far), read-only."""
    hop, nfft = ci.MODES[mode][2:4]
    lo, hi = ci.KEPT[nfft]
    pcm = stream(mode, name)
    o = ci.oracle(mode)
    out = []
    for k in range(0, len(pcm), hop):
        ci.push(o, mode, pcm[k:k + hop])
        whole = len(pcm) - k >= hop  # the estimator ran
        row = (o.coarse_absx()[lo:hi + 1].copy() if whole else None, o.coarse_y()[lo:hi + 1].copy(), o.hops().copy())
        for a in row:
            if a is not None:
                a.setflags(write=False)
        out.append(row)
    assert len(out[-1][2]) == len(pcm) // hop
    return out
