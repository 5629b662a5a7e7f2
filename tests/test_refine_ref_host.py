"""The CPU side of tests/test_gpu_refine_xref.py (tests/_refine_ref.py): the long-double back-substitution reproduces its right-hand
side, the Python double-double helpers are error-free, finish_model agrees with exact rational arithmetic -- and the NEGATIVE
CONTROLS that give the GPU tests their teeth: on every case of the GPU tables a plain fp64 product misses the residual pass's
bound and a plain fp64 sum misses the finish tolerance by two orders of magnitude, so a kernel whose double-double arithmetic
degraded to fp64 accuracy would fail there too.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from gptorch_amd import rng
from tests import _factor_ref as fr
from tests import _refine_ref as rr
from tests import _xref as xr

LD = xr.LD


@pytest.mark.parametrize("n", [129, 385])
@pytest.mark.parametrize("family", ["well", "graded10", "rbf_ill"])
def test_backsub_ref_reproduces_alpha(family, n):
    """backsub_ref times L^T gives alpha back to long-double rounding: |L^T a - alpha|_i <= n 2^-63 (|L|^T |a|)_i (twice the
    bound of the long-double substitution's backward error, as for kyy_a_bound); and the fp64 statements behind e64 solve the
    same system (their error in the metric is small, and not zero)."""
    A = fr.matrix(family, n)
    L = np.linalg.cholesky(A)
    alpha = fr.rhs(A, 3).T.copy()
    ref = rr.backsub_ref(L, alpha)
    assert ref.dtype == LD and ref.shape == (3, n)
    back = ref @ xr.ld(L)                                        # (L^T a)^T = a^T L
    bound = n * LD(2) ** -63 * (np.abs(ref) @ np.abs(xr.ld(L)))
    over = float(np.max(np.abs(back - xr.ld(alpha)) / bound))
    sd = np.sqrt(np.diag(A))
    e64 = rr.backsub_e64(L, alpha, ref, sd)
    print("XREF refine host backsub_ref %s-%d residual/bound %.3f e64 %.3g (%.1f u)" % (family, n, over, e64, e64 / fr.U))
    assert over <= 1.0
    assert 0.0 < e64 < 1e-6
    assert rr.backsub_metric(ref, ref, sd) == 0.0
    assert np.allclose(rr.row_scales(L), sd, rtol=1e-12, atol=0)


def test_backsub_model_runs_the_kernels_block_order():
    """one block: the model is s W; several blocks: the same as an unblocked fp64 solve to within the e64 it defines"""
    A = fr.well(300)
    L = np.linalg.cholesky(A)
    alpha = fr.rhs(A, 2).T.copy()
    one = rr.backsub_model64(L[:100, :100], alpha[:, :100])
    assert np.array_equal(one, alpha[:, :100] @ fr.lower_inverse64(L[:100, :100]))
    ref = rr.backsub_ref(L, alpha)
    assert rr.backsub_metric(rr.backsub_model64(L, alpha), ref, np.sqrt(np.diag(A))) < 64 * fr.U


def test_dd_helpers_are_error_free():
    """hi + lo of dd_fma equals acc + a b: exactly where the terms cannot overlap, and to 2^-104 relative in general (the one
    rounding of lo); two_sum's pair is exact always."""
    N = 2000
    a, b = rng.normal(8601, N), rng.normal(8602, N)
    hi = rng.normal(8603, N) * 10.0 ** (4 * rng.uniform(8604, N) - 2)
    lo = hi * 2.0 ** -54 * (2 * rng.uniform(8605, N) - 1)
    worst = 0.0
    for i in range(N):
        s, e = rr.two_sum(float(a[i]), float(b[i]))
        assert Fraction(s) + Fraction(e) == Fraction(float(a[i])) + Fraction(float(b[i]))
        p = float(a[i]) * float(b[i])
        assert Fraction(p) + Fraction(rr.fma(float(a[i]), float(b[i]), -p)) == Fraction(float(a[i])) * Fraction(float(b[i]))
        acc = (float(hi[i]), float(lo[i]))
        exact = Fraction(acc[0]) + Fraction(acc[1]) + Fraction(float(a[i])) * Fraction(float(b[i]))
        got = rr.dd_fma(acc, float(a[i]), float(b[i]))
        scale = abs(Fraction(acc[0])) + abs(Fraction(float(a[i])) * Fraction(float(b[i])))
        worst = max(worst, float(abs(Fraction(got[0]) + Fraction(got[1]) - exact) / scale))
        x = (float(b[i]), float(b[i]) * 2.0 ** -55)
        got = rr.dd_add(acc, x)
        exact = Fraction(acc[0]) + Fraction(acc[1]) + Fraction(x[0]) + Fraction(x[1])
        worst = max(worst, float(abs(Fraction(got[0]) + Fraction(got[1]) - exact) / (abs(Fraction(acc[0])) + abs(Fraction(x[0])))))
    print("XREF refine host dd_helpers random worst err/tol %.3f (2^-104 relative)" % (worst / 2.0 ** -104))
    assert worst <= 2.0 ** -104
    # a plain fp64 accumulation of the same pairs is not (the helpers are not vacuous)
    assert any(Fraction(float(hi[i]) + float(a[i]) * float(b[i])) != Fraction(float(hi[i])) + Fraction(float(a[i])) * Fraction(float(b[i]))
               for i in range(N))


@pytest.mark.parametrize("n,dy,with_m", rr.FINISH_CASES, ids=["%d-%d-%s" % (n, dy, "m" if w else "nom") for n, dy, w in rr.FINISH_CASES])
def test_finish_model_and_its_negative_control(n, dy, with_m):
    """On every case of the GPU finish table: the inputs cancel as built (|quad| <= 2^-20 S); finish_model agrees with
    finish_exact to 2 u |quad|; and the plain fp64 sum misses the finish tolerance by at least 100 x.

    One term (n dy = 1) cannot cancel, and no realistic input makes a plain fp64 evaluation of ONE product miss two roundings by
    two orders of magnitude: 2 (y - m) - ka_hi is exact or rounded once, - ka_lo and the product round once each, 3 u |quad| at
    most against a tolerance of 2 u |quad|.  There the control is asserted as that statement (the case tests the kernel's
    single-element path, bounds and the LML term; it cannot tell double-double from fp64, and nothing could)."""
    y, m, a, ka_hi, ka_lo = rr.cancelling_finish_inputs(n, dy, seed=n + dy)
    if not with_m:
        y, m = y - m, None
    quad, S = rr.finish_exact(y, m, a, ka_hi, ka_lo)
    r = (y - m) if m is not None else y
    assert float(np.max(np.abs(ka_hi + ka_lo - r.T) / np.abs(r.T))) < 1e-7          # as after a real step
    model = rr.finish_model(y, m, a, ka_hi, ka_lo)
    merr = rr.frac_err(model, quad)
    tol = rr.finish_tol(model, quad)
    miss = rr.frac_err(rr.finish_fp64(y, m, a, ka_hi, ka_lo), quad) / tol
    print("XREF refine host finish %d-%d-%s |quad|/S 2^%.1f model err/(2u|quad|) %.3g fp64 err/tol %.3g"
          % (n, dy, "m" if with_m else "nom", np.log2(float(abs(quad) / S)), merr / (2 * fr.U * abs(float(quad))), miss))
    assert merr <= 2 * fr.U * abs(float(quad))
    if n * dy == 1:
        assert abs(quad) == S and miss <= 1.5
        return
    assert abs(quad) <= S / 2 ** 20
    assert miss >= rr.FINISH_CONTROL_MISS


def test_finish_in_fp64_passes_on_data_that_does_not_cancel():
    """why the builder cancels: with random data a plain fp64 sum is within a few tolerances of the exact value -- a test on
    such data could not tell double-double from fp64."""
    n, dy = 1100, 3
    y, m, a, ka_hi, ka_lo = rr.cancelling_finish_inputs(n, dy, seed=5)
    a = rng.normal(8700, (dy, n))                                # nothing solved for
    quad, S = rr.finish_exact(y, m, a, ka_hi, ka_lo)
    model = rr.finish_model(y, m, a, ka_hi, ka_lo)
    miss = rr.frac_err(rr.finish_fp64(y, m, a, ka_hi, ka_lo), quad) / rr.finish_tol(model, quad)
    assert rr.frac_err(model, quad) <= 2 * fr.U * abs(float(quad))
    assert miss < rr.FINISH_CONTROL_MISS


@pytest.mark.parametrize("kind,n,d,ard,dy", rr.resid_cases(), ids=["%s-%d-%d-%d" % (k, n, d, dy) for k, n, d, _, dy in rr.resid_cases()])
def test_fp64_product_misses_the_residual_bound(kind, n, d, ard, dy):
    """On every case of the GPU residual-pass table (the same points and a; Kyy by direct differences in fp64 on the CPU where the
    GPU test takes the assembled matrix): numpy's fp64 product and a sequential one both miss kyy_a_bound."""
    xn, ls, a = rr.resid_inputs(kind, n, d, ard, dy)
    M = rr.kyy64(kind, xn, ls, rr.RESID_NOISE)
    assert np.array_equal(M, M.T)
    miss = rr.fp64_product_misses(M, a)
    print("XREF refine host resid_control %s-%d-%d-%d worst err/tol numpy %.3g sequential %.3g" % (kind, n, d, dy, miss[0], miss[1]))
    assert min(miss) > 1.0


def test_step_quad_exact_is_exact():
    """the dyadic-integer evaluation of sum a_i (2 r_i - (M a)_i) against fractions.Fraction entry by entry"""
    n, dy = 9, 2
    M = rng.normal(8801, (n, n)) * 10.0 ** (6 * rng.uniform(8802, n * n).reshape(n, n) - 3)
    M[2, 3] = 0.0
    r, a = rng.normal(8803, (dy, n)), rng.normal(8804, (dy, n))
    want = Fraction(0)
    for c in range(dy):
        for i in range(n):
            ma = sum(Fraction(float(M[i, j])) * Fraction(float(a[c, j])) for j in range(n))
            want += Fraction(float(a[c, i])) * (2 * Fraction(float(r[c, i])) - ma)
    assert rr.step_quad_exact(r, M, a) == want


def test_case_tables_cover_what_they_claim():
    cases = rr.resid_cases()
    for kind in rr.KIND_LIST:
        assert {(n, d, ard) for k, n, d, ard, _ in cases if k == kind} == set(rr.RESID_SHAPES)
        assert {dy for k, _, _, _, dy in cases if k == kind} == set(rr.RESID_DY)
    for shape in rr.RESID_SHAPES:
        assert {dy for _, n, d, ard, dy in cases if (n, d, ard) == shape} == set(rr.RESID_DY)
    assert len(rr.backsub_cases()) == (len(rr.BACKSUB_SIZES) + 2 * len(rr.BACKSUB_FAMILIES_AT)) * len(rr.BACKSUB_DY)
    x = rr.points(3, 80, 2, 0.5)
    assert np.array_equal(x[0], np.zeros(2)) and np.array_equal(x[21], x[1]) and x[28, 0] == 500.0
