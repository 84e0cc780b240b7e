"""aero_log10_ge1_tab (aero_math.h): log10 for finite arguments that are at
least 1, with the exponent and mantissa handling in 32-bit operations on the
high word, equals glibc's log10 by bit pattern: 1.0 itself, log's near-1 bound
1 + 0x1.09p-4 and both its neighbours in every binade, every power of two and
its neighbours, DBL_MAX, and 3 M log-uniform values over the whole range.
Host build (tools/mathhost.cpp); the device build against it is
tests/test_gpu_coarse_diet.py."""
import numpy as np

import coarse_diet_inputs as di
import mathhost


def _same(x):
    h = di.host_log10_ge1(x).view(np.int64)
    g = mathhost.glibc('log10', x).view(np.int64)
    bad = np.flatnonzero(h != g)
    assert bad.size == 0, (bad.size, x[bad[:4]], h[bad[:4]], g[bad[:4]])


def test_boundary_set_is_what_it_says(cpu_libs):
    x = di.boundary_set()
    bits = x.view(np.uint64)
    assert 1.0 in x and np.finfo(np.float64).max in x
    for k in (0, 1, 52, 1023):
        p = np.float64(2.0) ** k
        assert p in x and np.nextafter(p, np.inf) in x and (k == 0 or np.nextafter(p, 0.0) in x)
        b = np.uint64(di.NEAR_HI) + (np.uint64(k) << np.uint64(52))
        assert all(v in bits for v in (b - np.uint64(1), b, b + np.uint64(1)))
    near = di.near1(x)
    b = np.uint64(di.NEAR_HI) + (np.arange(1024, dtype=np.uint64) << np.uint64(52))
    assert di.near1((b - np.uint64(1)).view(np.float64)).all() and not di.near1(b.view(np.float64)).any()
    assert near.any() and not near.all()


def test_log10_ge1_boundaries_bit_exact(cpu_libs):
    x = di.boundary_set()
    _same(x)
    assert di.host_log10_ge1(np.array([1.0]))[0] == 0.0 and not np.signbit(di.host_log10_ge1(np.array([1.0]))[0])


def test_log10_ge1_log_uniform_bit_exact(cpu_libs):
    rng = np.random.default_rng(0x10610)
    x = np.exp2(rng.uniform(0.0, 1023.0, 3_000_000))
    assert x.min() >= 1.0 and np.isfinite(x).all()
    _same(x)
    # and the estimator's own range with the mantissa drawn around the bound
    m = 1.0 + rng.uniform(0.0, 0.13, 400_000)
    _same(m * np.exp2(rng.integers(0, 64, m.size)))


def test_log10_ge1_equals_the_general_function(cpu_libs):
    """The same bits as aero_log10 (what the kernel ran before), not only as glibc."""
    x = np.concatenate([di.boundary_set(), np.exp2(np.random.default_rng(5).uniform(0.0, 1023.0, 200_000))])
    assert np.array_equal(di.host_log10_ge1(x).view(np.int64), mathhost.evaluate('log10', x).view(np.int64))
