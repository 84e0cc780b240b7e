"""Seeded input records for the device FFTs (aero_device_fft) and their
reference, the oracle's JFFT (oracle_fft), composed as
tests/test_fft_chain_sim.py composes it.  tests/test_fft_inputs.py runs the
chain records through the host model of the kernel's layouts on the CPU,
tests/test_gpu_fft.py through the device code.

Classes (every transform size gets every class):
  prod      CIS x pcm / 32768 with 100 leading zeros, the coarse estimator's input
  impulse   one unit value (real 1, imaginary 1, (1, 1)) at the first, middle
            and last positions and 16 random ones: every output is a chain of
            twiddle products without cancellation
  tone      one complex exponential on a bin: one bin holds the energy, exact
            and near cancellation everywhere else
  uniform   [-1, 1)^2, and the same values times 2^+e and 2^-e (e = 400; 200
            where the chain squares, which doubles the exponent)
  zeros     all zero, and zeros with negative signs sprinkled in
  full      alternating +-(1, -1), and the constant (-1, -1)
"""
import functools

import numpy as np

import aero_testlib as tl

SEED = 0xFF7
DIT = [(12, False), (12, True), (13, False), (13, True), (14, False)]  # fft_dit<L, INV> as production builds it
CHAIN_L = (13, 14)


def chain_limits(log2n):
    """(start, stop) of the boxcar: the production sets (OQPSK at 16384; MSK at
    12000, 24000 and 48000 Hz at 8192), then none, one bin, all but bin 0."""
    n = 1 << log2n
    prod = {14: [(3584, 12800)], 13: [(614, 7578), (307, 7885), (154, 8038)]}[log2n]
    return prod + [(1, 0), (n // 2, n // 2), (1, n - 1)]


def scale_exp(depth):
    return 200 if depth == 3 else 400


@functools.lru_cache(maxsize=None)
def records(n, exp=400):
    """(labels, [nrec, n] complex128, read-only).  A label is (class, detail);
    the uniform class's are ('uniform', 0), ('uniform', +exp), ('uniform', -exp)."""
    rng = np.random.default_rng([SEED, n])
    labels, rows = [], []

    def add(cls, detail, x):
        labels.append((cls, detail))
        rows.append(np.asarray(x, dtype=np.complex128))

    cis = np.exp(1j * rng.uniform(0, 2 * np.pi, n))
    pcm = rng.integers(-32768, 32768, n) / 32768.0
    pcm[:100] = 0
    add('prod', 0, cis * pcm)
    pos = [0, 1, 2, n // 2 - 1, n // 2, n - 2, n - 1] + sorted(int(p) for p in rng.choice(n, 16, replace=False))
    for v in (1.0, 1j, 1.0 + 1j):
        for p in pos:
            x = np.zeros(n, dtype=np.complex128)
            x[p] = v
            add('impulse', (p, v), x)
    j = np.arange(n)
    for k in [0, 1, n // 4, n // 2, n - 1] + sorted(int(b) for b in rng.choice(n, 8, replace=False)):
        add('tone', k, np.exp(2j * np.pi * ((k * j) % n) / n))
    u = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    add('uniform', 0, u)
    add('uniform', exp, scaled(u, exp))
    add('uniform', -exp, scaled(u, -exp))
    add('zeros', 'plus', np.zeros(n))
    z = np.zeros(n, dtype=np.complex128)
    z.real[rng.random(n) < 0.3] = -0.0
    z.imag[rng.random(n) < 0.3] = -0.0
    assert np.signbit(z.real).any() and np.signbit(z.imag).any() and not np.signbit(z.real).all()
    add('zeros', 'signed', z)
    alt = np.where(j % 2 == 0, 1.0, -1.0)
    add('full', 'alternating', alt - 1j * alt)
    add('full', 'constant', np.full(n, -1.0 - 1.0j))
    arr = np.stack(rows)
    arr.setflags(write=False)
    return tuple(labels), arr


def scaled(x, k):
    """x times 2^k, each part by itself (exact; no complex product)."""
    out = np.empty(x.shape, dtype=np.complex128)
    out.real, out.imag = x.real * 2.0 ** k, x.imag * 2.0 ** k
    return out


def _fft(x, n, inverse):
    tl.Oracle.lib().oracle_fft(x.ctypes.data, n, 1 if inverse else 0)


def ref_dit(rows, inverse):
    """JFFT per row; the inverse times N (the device leaves JFFT's 1/N out; exact)."""
    n = rows.shape[1]
    out = np.empty_like(rows)
    for r, x in enumerate(rows):
        y = x.copy()
        _fft(y, n, inverse)
        out[r] = scaled(y, n.bit_length() - 1) if inverse else y
    return out


@functools.lru_cache(maxsize=None)
def _forward(n, exp):
    rows = records(n, exp)[1]
    out = np.empty_like(rows)
    for r, x in enumerate(rows):
        y = x.copy()
        _fft(y, n, False)
        out[r] = y
    out.setflags(write=False)
    return out


def ref_chain(n, exp, depth, start, stop):
    """Of records(n, exp): forward; bins start..stop zeroed, inverse, x N
    (FFTWrapper; exact); the square from separate products (numpy's complex
    product may fuse), forward.  The forward transforms are computed once."""
    fwd = _forward(n, exp)
    if depth == 1:
        return fwd
    out = np.empty_like(fwd)
    for r, x in enumerate(fwd):
        y = x.copy()
        y[start:stop + 1] = 0
        _fft(y, n, True)
        y = scaled(y, n.bit_length() - 1)
        if depth >= 3:
            re, im = y.real.copy(), y.imag.copy()
            y = np.empty(n, dtype=np.complex128)
            y.real, y.imag = re * re - im * im, re * im + im * re
            _fft(y, n, False)
        out[r] = y
    return out


def thinned(labels):
    """Row indices of a smaller set with every class in it: every fourth
    impulse and everything else (for the slow host model's further limits)."""
    imp = [i for i, l in enumerate(labels) if l[0] == 'impulse']
    return np.array(sorted(set(range(len(labels))) - set(imp) | set(imp[::4])))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def differing(got, ref, bitwise):
    """Per row the indices of the values that differ: by bit pattern, or by
    value (+-0 equal) with any NaN on either side counting as a difference."""
    if bitwise:
        bad = (_bits(got.real) != _bits(ref.real)) | (_bits(got.imag) != _bits(ref.imag))
    else:
        bad = (got.real != ref.real) | (got.imag != ref.imag)  # NaN != anything
    return bad


def check(what, labels, got, ref, bitwise):
    """Asserts got == ref; the message names the transform (`what`: kind, N,
    direction or depth and limits), class, detail, seed, first differing
    index and the number of differing values of up to 8 records."""
    assert got.shape == ref.shape
    if not bitwise:
        assert not np.isnan(ref.real).any() and not np.isnan(ref.imag).any(), '%s: NaN in the reference' % what
    bad = differing(got, ref, bitwise)
    rows = np.flatnonzero(bad.any(axis=1))
    msg = ['%s seed %#x class %s %s: first differing index %d, %d of %d values differ' %
           (what, SEED, labels[r][0], labels[r][1], int(np.flatnonzero(bad[r])[0]), int(bad[r].sum()), bad.shape[1])
           for r in rows[:8]]
    assert not len(rows), '%d records differ\n' % len(rows) + '\n'.join(msg)


def check_scaling(what, labels, got, exp, factor_exp, bitwise):
    """The uniform class's scaled outputs equal the unscaled output times
    2^+-factor_exp exactly (a self-check that needs no reference)."""
    at = {l: i for i, l in enumerate(labels)}
    base = got[at['uniform', 0]]
    for sgn in (1, -1):
        want = scaled(base, sgn * factor_exp)
        assert np.isfinite(want.real).all() and np.isfinite(want.imag).all()
        r = at['uniform', sgn * exp]
        check('%s scaled by 2^%d against unscaled' % (what, sgn * exp), labels[r:r + 1], got[r:r + 1], want[None, :],
              bitwise)
