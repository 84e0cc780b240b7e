"""The records of tests/fft_inputs.py and its reference composition, proven on
the CPU before a GPU sees them: the host model of the coarse kernel's chained
transforms (tools/fft_chain_sim.cpp: the kernel's layouts, twiddle indices,
permuted twiddle copy and trivial-twiddle skips) gives, for every record,
depth and boxcar limit that tests/test_gpu_fft.py hands to the device, what
the oracle's JFFT chain gives, up to the sign of exact zeros, and the scaled
records give the unscaled result times the power of two."""
import ctypes
import os

import numpy as np
import pytest

import aero_testlib as tl
import fft_inputs as fi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = os.path.join(ROOT, 'tools', 'libfft_chain_sim.so')


def _sim_chain(log2n, rows, depth, start, stop):
    n = 1 << log2n
    L = ctypes.CDLL(SIM)
    L.fft_chain_sim_depth.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    O = tl.Oracle.lib()
    tw, twi = np.zeros(2 * n), np.zeros(2 * n)
    O.oracle_twiddles(n, 0, tw.ctypes.data)
    O.oracle_twiddles(n, 1, twi.ctypes.data)
    rows = np.ascontiguousarray(rows)
    out = np.zeros_like(rows)
    assert L.fft_chain_sim_depth(log2n, tw.ctypes.data, twi.ctypes.data, rows.ctypes.data, rows.shape[0], start, stop,
                                 depth, out.ctypes.data) == 0
    return out


def test_record_set_holds_every_class():
    for log2n in (12, 13, 14):
        for exp in (400, 200):
            labels, rows = fi.records(1 << log2n, exp)
            assert rows.shape == (len(labels), 1 << log2n) and len(set(labels)) == len(labels)
            count = {c: sum(1 for l in labels if l[0] == c) for c in ('prod', 'impulse', 'tone', 'uniform', 'zeros',
                                                                       'full')}
            assert count == {'prod': 1, 'impulse': 69, 'tone': 13, 'uniform': 3, 'zeros': 2, 'full': 2}
            assert np.isfinite(rows.real).all() and np.isfinite(rows.imag).all()
            assert {labels[i][0] for i in fi.thinned(labels)} == set(count) and len(fi.thinned(labels)) == 39


@pytest.mark.parametrize('log2n', fi.CHAIN_L)
@pytest.mark.parametrize('depth', [1, 2, 3])
def test_chain_model_equals_reference(log2n, depth, cpu_libs):
    n, exp = 1 << log2n, fi.scale_exp(depth)
    labels, rows = fi.records(n, exp)
    for k, (start, stop) in enumerate(fi.chain_limits(log2n) if depth > 1 else [(1, 0)]):
        what = 'chain model N %d depth %d limits %d..%d' % (n, depth, start, stop)
        # the model takes 25 ms per record: every record at the first limits, a
        # thinned set (every class still) at the others
        keep = np.arange(len(labels)) if k == 0 else fi.thinned(labels)
        lab = [labels[i] for i in keep]
        got = _sim_chain(log2n, rows[keep], depth, start, stop)
        fi.check(what, lab, got, fi.ref_chain(n, exp, depth, start, stop)[keep], bitwise=False)
        fi.check_scaling(what, lab, got, exp, 2 * exp if depth == 3 else exp, bitwise=False)


def test_checks_notice_a_difference():
    """One value off by an ulp, a NaN, and (bitwise only) the sign of a zero."""
    labels, rows = fi.records(4096)
    ref = np.array(rows[:3])
    for bitwise in (False, True):
        got = ref.copy()
        got.real[1, 7] = np.nextafter(got.real[1, 7], 2.0)
        with pytest.raises(AssertionError, match='first differing index 7, 1 of 4096'):
            fi.check('x', labels, got, ref, bitwise)
        got = ref.copy()
        got.imag[2, 5] = np.nan
        with pytest.raises(AssertionError, match='first differing index 5'):
            fi.check('x', labels, got, ref, bitwise)
    z = np.zeros((1, 8), dtype=np.complex128)
    m = z.copy()
    m.real[0, 3] = -0.0
    fi.check('x', labels, m, z, bitwise=False)
    with pytest.raises(AssertionError, match='first differing index 3'):
        fi.check('x', labels, m, z, bitwise=True)
