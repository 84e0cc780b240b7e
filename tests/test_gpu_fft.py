"""The device FFTs against the oracle's JFFT, value for value:
aero_device_fft runs fft_dit<L, INV> (csrc/fft_dit.h: the C channel's
prefilter, the burst Hilbert fast-FIR, the trident check) and the coarse
estimator's chained transforms (csrc/fft_chain.h, at a depth of 1, 2 and 3)
on the records of tests/fft_inputs.py, with tables built by the functions
the channel groups use.  No tolerances: fft_dit's bit patterns equal the
oracle's; the chain's values equal them with +-0 taken as equal (it skips the
exact (1, +-0) twiddle products) and hold no NaN.  The scaled
uniform records must also give the unscaled result times the power of two.
tests/test_fft_inputs.py proves the records and the reference on the CPU."""
import numpy as np
import pytest

import aero_testlib as tl  # noqa: F401  (puts the package on sys.path)
import fft_inputs as fi


@pytest.fixture(scope='module')
def eng(engine_lib):
    import aero_engine as ae
    e = ae.Engine(max_channels=1)
    yield e
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize('log2n,inverse', fi.DIT)
def test_dit_equals_oracle_bit_for_bit(eng, log2n, inverse):
    n = 1 << log2n
    labels, rows = fi.records(n)
    what = 'dit N %d %s' % (n, 'inverse' if inverse else 'forward')
    got = eng.device_fft('dit', rows, inverse=inverse)  # every record of this kind and N in one launch
    fi.check(what, labels, got, fi.ref_dit(rows, inverse), bitwise=True)
    fi.check_scaling(what, labels, got, 400, 400, bitwise=True)


@pytest.mark.gpu
@pytest.mark.parametrize('log2n', fi.CHAIN_L)
@pytest.mark.parametrize('depth', [1, 2, 3])
def test_chain_equals_oracle(eng, log2n, depth):
    n, exp = 1 << log2n, fi.scale_exp(depth)
    labels, rows = fi.records(n, exp)
    for start, stop in (fi.chain_limits(log2n) if depth > 1 else [(1, 0)]):
        what = 'chain N %d depth %d limits %d..%d' % (n, depth, start, stop)
        got = eng.device_fft('chain', rows, depth=depth, start=start, stop=stop)
        fi.check(what, labels, got, fi.ref_chain(n, exp, depth, start, stop), bitwise=False)
        fi.check_scaling(what, labels, got, exp, 2 * exp if depth == 3 else exp, bitwise=False)


@pytest.mark.gpu
def test_chain_depth1_ignores_the_limits(eng):
    """The boxcar belongs to depth 2: a depth-1 call with limits set is the plain forward transform."""
    labels, rows = fi.records(8192)
    keep = fi.thinned(labels)
    got = eng.device_fft('chain', rows[keep], depth=1, start=1, stop=8191)
    fi.check('chain N 8192 depth 1 limits 1..8191', [labels[i] for i in keep], got,
             fi.ref_chain(8192, 400, 1, 1, 0)[keep], bitwise=False)


@pytest.mark.gpu
def test_probe_refuses_what_it_cannot_run(eng):
    import aero_engine as ae
    ok = np.zeros((1, 8192), dtype=np.complex128)
    for kind, rows, kw in (('dft', ok, {}),                                   # unknown kind
                           ('dit', np.zeros((1, 2048), dtype=np.complex128), {}),  # no 2048-point transform
                           ('dit', np.zeros((1, 6000), dtype=np.complex128), {}),  # not a power of two
                           ('dit', np.zeros((1, 16384), dtype=np.complex128), {'inverse': True}),  # not built
                           ('chain', np.zeros((1, 4096), dtype=np.complex128), {'depth': 1}),  # the chain: 13, 14
                           ('chain', ok, {'depth': 0}), ('chain', ok, {'depth': 4}),
                           ('chain', ok, {'depth': 1, 'inverse': True}),
                           ('dit', np.zeros((257, 4096), dtype=np.complex128), {})):  # above the record cap
        with pytest.raises(ae.AeroError) as ei:
            eng.device_fft(kind, rows, **kw)
        assert ei.value.rc == ae.AERO_E_INVALID, (kind, rows.shape, kw)
    assert eng.device_fft('dit', np.zeros((256, 4096), dtype=np.complex128)).shape == (256, 4096)  # the cap itself runs
