"""A numpy emulation of ONE float32 fused multiply-add, correctly rounded — the unit every SpMM accumulation step is
made of (gcr_spmm.hip: one `fmaf` per stored non-zero, in stored order, from 0).  tests/test_spmm_pipeline_gpu.py replays
the kernel's documented order with it and demands equal bits, so the emulation itself is checked here against exact
rational arithmetic.

How it works: the product of two float32 is exact in float64 (48 significant bits); TwoSum with the addend gives the
float64 sum and its exact error; when the error is non-zero the sum is moved onto the neighbour with an odd last bit
(round to odd), which makes the final cast to float32 (29 bits fewer) round as if from the exact value."""
from fractions import Fraction

import numpy as np

F32, F64 = np.float32, np.float64


def fma32(a, b, c):
    """float32(a * b + c) with a single rounding, elementwise (numpy broadcasting)."""
    a, b, c = (np.asarray(t, dtype=F32).astype(F64) for t in (a, b, c))
    p = a * b                                   # exact
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)             # TwoSum: p + c = s + err exactly
    s = np.atleast_1d(s).copy()
    err = np.broadcast_to(err, s.shape)
    bits = s.view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s[fix] = np.nextafter(s[fix], np.broadcast_to(toward, s.shape)[fix])
    with np.errstate(over="ignore"):
        out = s.astype(F32)
    return out.reshape(np.broadcast(a, b, c).shape)


def _round_f32_exact(v: Fraction) -> np.float32:
    """Fraction -> nearest float32, ties to even, subnormals included (no overflow handling: callers stay in range)."""
    if v == 0:
        return F32(0.0)
    sign = -1 if v < 0 else 1
    m = abs(v)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    if Fraction(2) ** e > m:
        e -= 1
    assert Fraction(2) ** e <= m < Fraction(2) ** (e + 1)
    q = Fraction(2) ** (max(e, -126) - 23)
    n = m / q
    lo = n.numerator // n.denominator
    rem = n - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    return F32(sign * float(Fraction(lo) * q))      # lo * q has <= 24 significant bits: the conversion is exact


def _check(a, b, c):
    got = fma32(a, b, c)
    for i in range(a.size):
        want = _round_f32_exact(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert got[i].view(np.uint32) == want.view(np.uint32) or (got[i] == 0 and want == 0), \
            (float(a[i]), float(b[i]), float(c[i]), float(got[i]), float(want))


def test_fma32_random_triples_match_exact_rational_arithmetic():
    rng = np.random.default_rng(0)
    n = 3000
    a = rng.standard_normal(n).astype(F32)
    b = rng.standard_normal(n).astype(F32)
    c = rng.standard_normal(n).astype(F32)
    _check(a, b, c)
    # wide exponent spread: the addend dwarfs the product and the other way round
    sc = lambda: (2.0 ** rng.integers(-40, 40, n)).astype(F32)
    _check(a * sc(), b * sc(), c * sc())


def test_fma32_cancellation_and_ties():
    rng = np.random.default_rng(1)
    n = 1500
    a = rng.standard_normal(n).astype(F32)
    b = rng.standard_normal(n).astype(F32)
    prod = (a.astype(F64) * b.astype(F64))
    c = (-prod).astype(F32)                      # a*b + c cancels to the product's own rounding error
    _check(a, b, c)
    c2 = np.nextafter(c, F32(np.inf))
    _check(a, b, c2)
    # exact ties of the float32 result: 1 + k * 2^-24 for odd k sits halfway between two float32
    k = np.arange(1, 64, 2).astype(F32)
    _check(k, np.full_like(k, F32(2.0 ** -24)), np.ones_like(k))
    _check(k, np.full_like(k, F32(-2.0 ** -24)), np.ones_like(k))
    # a tie broken only by a term far below the float64 sum's last bit (double rounding would get this wrong)
    one = np.ones(4, F32)
    tiny = np.array([2.0 ** -60, -2.0 ** -60, 2.0 ** -100, -2.0 ** -100], F32)
    _check(tiny, one, one * F32(1.0 + 2.0 ** -23))
    a3 = np.array([2.0 ** -24 + 2.0 ** -47, 2.0 ** -24 - 2.0 ** -48, 2.0 ** -24 + 2.0 ** -47, 2.0 ** -24], F32)
    _check(a3, np.array([1, 1, -1, -1], F32), np.array([1, 1, 3, 3], F32))
    # product carries the tie-breaking bit 2^-76 below a sum near 1: outside float64's 53 bits, kept by round to odd
    a4 = np.array([1 + 2.0 ** -23, 1 + 2.0 ** -23, -(1 + 2.0 ** -23)], F32)
    b4 = np.array([2.0 ** -24 + 2.0 ** -47, 2.0 ** -24, 2.0 ** -24 + 2.0 ** -47], F32)
    _check(a4 * F32(2.0 ** -30), b4 * F32(2.0 ** 30), np.array([1, 1, 1], F32))
    _check(np.array([2.0 ** -64, 2.0 ** -64], F32), np.array([1 + 2.0 ** -23, 1], F32) * F32(2.0 ** 40), np.array([1, 1], F32))


def test_fma32_subnormal_results_and_inputs():
    rng = np.random.default_rng(2)
    n = 1000
    a = (rng.standard_normal(n) * 2.0 ** -70).astype(F32)
    b = (rng.standard_normal(n) * 2.0 ** -70).astype(F32)
    c = (rng.standard_normal(n) * 2.0 ** -140).astype(F32)      # subnormal addends, subnormal results
    assert (np.abs(c) < np.finfo(F32).tiny).all()
    _check(a, b, c)
    _check(a, b, np.zeros(n, F32))
    tiny = np.finfo(F32).tiny
    _check(np.full(8, tiny, F32), np.linspace(0.1, 0.9, 8).astype(F32), np.full(8, -tiny / 2, F32))
    sub = np.array([1e-45, 3e-45, -1e-45, 7e-42], F32)          # subnormal inputs
    _check(sub, np.array([0.5, 1.5, 0.75, 1.25], F32), np.array([1e-45, -1e-45, 0, 3e-44], F32))
