"""The yardsticks of tests/test_gpu_factor_xref.py, checked on the CPU: the matrix families are what they claim to be, the fp64
model of the kernels' algorithm (tests/_factor_ref.py) reproduces the long-double factor as well as LAPACK does where the two
should agree, and the planted failures have the pivot index that LAPACK reports."""
import numpy as np
import pytest
import torch

from tests import _factor_ref as fr
from tests import _xref as xr

N = 385          # three leaf blocks, ragged last one


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(family):
        if family not in cache:
            A = fr.matrix(family, N)
            cache[family] = (A, fr.FactorRef(A, fr.rhs(A, 3)))
        return cache[family]
    return get


@pytest.mark.parametrize("family", ["well", "graded2", "graded10"])
def test_model_matches_lapack_where_they_should_agree(refs, family):
    """forward error, residual, extra rows and leaf inverses of the fp64 model within 16 x LAPACK's error (floor 8 u)"""
    A, ref = refs(family)
    R = ref.R
    Lm, Em, Wm = fr.model_factor(A, R)
    Ll, El, Wl = fr.lapack_factor(A, R)
    for what, fn, gm, gl in (("forward", ref.forward, Lm, Ll), ("residual", ref.residual, Lm, Ll), ("extra", ref.extra_err, Em, El)):
        em, el = fn(gm), fn(gl)
        print("%s %s: model %.2f u, LAPACK %.2f u" % (family, what, em / fr.U, el / fr.U))
        assert em <= fr.tol(el), (what, em, el)
    for k, (em, el) in enumerate(zip(ref.leaf_errs(Wm), ref.leaf_errs(Wl))):
        assert em <= fr.tol(el), ("leaf", k, em, el)
    assert np.array_equal(np.triu(Lm, 1), np.zeros_like(Lm))


def test_graded2_scales_the_model_exactly():
    """D = diag(2^k) scales every fp64 operation of the model exactly: its factor of graded2 is D times its factor of well, bit for
    bit, and the extra rows are the same bits (the property the GPU kernels are held to)."""
    A0, A2 = fr.well(N), fr.graded2(N)
    d = np.ldexp(1.0, fr.graded2_exponents(N))
    assert np.array_equal(A2, A0 * d[:, None] * d[None, :]) and np.array_equal(A2, A2.T)
    R0 = fr.rhs(A0, 3)
    R2 = fr.rhs(A2, 3)
    assert np.array_equal(R2, R0 * d[:, None])
    # (numpy's own Cholesky of the diagonal blocks is LAPACK: its sqrt and divisions scale exactly as well)
    L0, E0, W0 = fr.model_factor(A0, R0)
    L2, E2, W2 = fr.model_factor(A2, R2)
    assert np.array_equal(L2, L0 * d[:, None])
    assert np.array_equal(E2, E0)
    for b in range(W0.shape[0]):
        k = b * fr.LEAF
        c = min(k + fr.LEAF, N)
        assert np.array_equal(W2[b, :c - k, :c - k], W0[b, :c - k, :c - k] / d[None, k:c])


def test_condition_numbers():
    assert fr.cond2(fr.well(N)) < 50
    assert 1e7 < fr.cond2(fr.rbf_ill(N)) < 1e10
    assert 1e7 < fr.cond2(fr.rbf_ill(1100)) < 1e10


@pytest.mark.parametrize("family", fr.FAMILIES)
def test_families_are_positive_definite_in_long_double(refs, family):
    A, ref = refs(family)                                           # xr.cholesky raises on a non-positive pivot
    assert np.array_equal(A, A.T)
    assert np.all(np.diag(ref.L) > 0)
    assert ref.ref_residual() < fr.U / 16                           # what `residual` leaves out is far below its 8 u floor


def test_residual_identity_against_the_direct_product(refs):
    """FactorRef.residual (through L - L_ref) equals the residual formed directly in long double"""
    for family in ("graded2", "rbf_ill"):
        A, ref = refs(family)
        L = fr.lapack_factor(A)[0]
        Ll = xr.ld(L)
        P = np.tril(np.einsum("ik,jk->ij", Ll, Ll) - xr.ld(A)) / ref.sd[:, None] / ref.sd[None, :]
        direct = float(np.max(np.abs(P)))
        assert abs(ref.residual(L) - direct) < fr.U / 8, (family, ref.residual(L), direct)


def test_triangular_family_is_not_a_cholesky_factor():
    for n in (1, 127, 129, 300):
        T = fr.triangular(n)
        assert np.array_equal(np.triu(T, 1), np.zeros_like(T))
        d = np.abs(np.diag(T))
        assert np.all(d >= 1.0) and np.all(d < 2.0)
        if n > 1:
            assert (np.diag(T) < 0).any() and (np.diag(T) > 0).any()


@pytest.mark.parametrize("pivots,nans", fr.planted_cases(), ids=fr.planted_ids())
def test_planted_failures_have_the_expected_index(pivots, nans):
    P, expect = fr.planted(fr.INFO_N, pivots, nans)
    assert np.all(np.linalg.eigvalsh(fr.well(fr.INFO_N)) >= 0.5)
    info = int(torch.linalg.cholesky_ex(torch.tensor(P)).info.item())
    assert info == expect
