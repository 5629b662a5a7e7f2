"""The yardstick of tests/test_gpu_gemm_xref.py, checked on the CPU: the long-double reference of tests/_gemm_ref.py against exact
rational arithmetic, the a-priori bound against numpy's own fp64 product on every family and shape the GPU module runs (it is
never tighter than a correct fp64 product needs), the masks against plain loops and the families against their definitions."""
from fractions import Fraction

import numpy as np
import pytest

from tests import _gemm_ref as gr

LD = gr.LD


def test_long_double_is_wider_than_fp64():
    """the reference's own error must be far below the bound: 64-bit mantissa, exponent range beyond 2^-1200"""
    assert np.finfo(LD).nmant >= 63 and np.finfo(LD).minexp <= -16000


def _frac(x):
    """a long double as an exact rational (its 64-bit mantissa as an integer; no detour through fp64, which would underflow on
    the `tiny` family)"""
    m, e = np.frexp(LD(x))
    n = int(np.ldexp(m, 64))
    assert np.ldexp(LD(n), int(e) - 64) == LD(x)
    return Fraction(n) * Fraction(2) ** (int(e) - 64)


def _exact(A, B, C0, alpha, beta):
    M, N = A.shape[0], B.shape[0]
    fa = [[Fraction(float(x)) for x in row] for row in A]
    fb = [[Fraction(float(x)) for x in row] for row in B]
    out = [[Fraction(alpha) * sum(x * y for x, y in zip(fa[i], fb[j])) + Fraction(beta) * Fraction(float(C0[i, j]))
            for j in range(N)] for i in range(M)]
    return out


@pytest.mark.parametrize("family", gr.FAMILIES)
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (0.37, -0.5)])
def test_ref_nt_against_exact_rationals(family, alpha, beta):
    """9 x 7 x 32: every product and sum exact in fractions.Fraction; the long-double reference is within (K + 3) 2^-63 S of it,
    i.e. 2^-10 of the bound it is used with"""
    M, N, K = 9, 7, 32
    A, B, C0 = gr.family(family, M, N, K)
    ref, S = gr.ref_nt(A, B, C0, alpha, beta)
    ex = _exact(A, B, C0, alpha, beta)
    worst = 0.0
    for i in range(M):
        for j in range(N):
            # |ref - exact| and the limit as exact rationals (S itself is rounded: 2^-50 of slack)
            err = abs(_frac(ref[i, j]) - ex[i][j])
            s = _frac(S[i, j])
            lim = Fraction(K + 3) * Fraction(2) ** -63 * s * Fraction(1 + 2.0 ** -50)
            assert err <= lim, (i, j, float(err), float(lim))
            if s > 0:
                worst = max(worst, float(err / (Fraction(2) ** -64 * s)))
    assert np.all(S > 0) or family == "tri"
    print("%s (%g, %g): worst reference error %.2f x 2^-64 S" % (family, alpha, beta, worst))


def _numpy_inside(A, B, C0, alpha, beta, P, SP, K, tiny, mask=None):
    ref, S = gr.combine(P, SP, C0, alpha, beta, mask)
    got = alpha * (A @ B.T) + (beta * C0 if beta != 0.0 else 0.0)
    if mask is not None:
        got = np.where(mask, got, C0)
    err = np.abs(gr.ld(got) - ref)
    assert np.all(err <= gr.bound(K, S, tiny)), (A.shape, B.shape, alpha, beta, int(np.sum(err > gr.bound(K, S, tiny))))
    return gr.units(got, ref, S, K, tiny)


@pytest.mark.parametrize("family", gr.FAMILIES)
def test_numpy_fp64_is_inside_the_bound_on_every_gpu_shape(family):
    """alpha (A @ B.T) + beta C0 in numpy fp64 (BLAS sums in its own order, alpha and beta applied with two more roundings than the
    kernel's fma) stays within bound(K, S, tiny) on every shape of the GPU module and every (alpha, beta)"""
    worst = 0.0
    shapes = list(gr.SHAPES) + [(n, n, K) for n, K in gr.LOWER1] + list(gr.LOWER2) + list(gr.TRI_SHAPES) + list(gr.THIN_SHAPES) \
        + [(M, nb * gr.STAIR_BLK, gr.STAIR_K) for M, nb, _, _ in gr.STAIR] + [gr.BATCH_SHAPE]
    for M, N, K in shapes:
        A, B, C0, P, SP = gr.case(family, M, N, K)
        for alpha, beta in gr.PAIRS:
            worst = max(worst, _numpy_inside(A, B, C0, alpha, beta, P, SP, K, gr.tiny_of(family, K)))
    print("%s: numpy fp64 worst err / (2^-53 S) = %.2f" % (family, worst))
    assert worst > 0.0


def test_numpy_fp64_is_inside_the_bound_on_the_other_inputs():
    """the flag sweep's operands, the split-K parts and matmul_nt's odd K"""
    for M, N, K in gr.TRI_SHAPES:
        for flags in range(1, 16):
            A, B, C0 = gr.tri(M, N, K, flags)
            P, SP = gr.product_ld(A, B)
            _numpy_inside(A, B, C0, 1.0, 0.0, P, SP, K, 0.0)
    for K in gr.MATMUL_K:
        A, B, C0 = gr.scaled(33, 18, K)
        P, SP = gr.product_ld(A, B)
        _numpy_inside(A, B, C0, -0.75, 0.0, P, SP, K, 0.0)


def test_families_are_what_they_claim():
    M, N, K = 31, 129, 48
    A, B, C0 = gr.scaled(M, N, K)
    ea, eb = np.frexp(np.abs(A).max(axis=1))[1], np.frexp(np.abs(B).max(axis=1))[1]
    assert ea.max() - ea.min() > 40 and eb.max() - eb.min() > 40 and ea.max() <= 44 and ea.min() >= -42
    # full mantissas: the low bit is set in about half of the entries
    low = (A.view(np.uint64) & np.uint64(1)).mean()
    assert 0.3 < low < 0.7
    At, Bt, Ct = gr.tiny(M, N, K)
    prod = np.abs(gr.ld(At[:, :1]) * gr.ld(Bt[:, 0])[None, :])
    assert np.all(np.abs(At) < 2.0 ** -470) and np.all(np.abs(At) >= 2.0 ** -580)
    assert np.mean(prod < LD(2.0) ** -1022) > 0.5               # most products are subnormal or below in fp64
    A, B, C0 = gr.cancel(M, N, K)
    assert np.array_equal(A[:, 0::2], A[:, 1::2])
    r = -B[:, 1::2] / B[:, 0::2] - 1.0
    assert np.all(r > 0.5e-10) and np.all(r < 2.5e-10)
    ref, S = gr.ref_nt(A, B)
    assert float(np.median(S / np.abs(ref))) > 1e9
    for flags in range(1, 16):
        A, B, _ = gr.tri(20, 30, 32, flags)
        for X, up, lo in ((A, gr.TRI_A_UPPER, gr.TRI_A_LOWER), (B, gr.TRI_B_UPPER, gr.TRI_B_LOWER)):
            for i in range(X.shape[0]):
                for k in range(X.shape[1]):
                    zero = bool(flags & up and k < i) or bool(flags & lo and k > i)
                    assert (X[i, k] == 0.0) == zero
    X = gr.dense_to_edge(200, 208)
    assert X[5, 127] != 0.0 and X[5, 128] == 0.0 and X[130, 207] != 0.0
    Y = gr.clip_to_tile(X, 32)
    assert Y[5, 31] != 0.0 and Y[5, 32] == 0.0 and Y[40, 63] != 0.0 and Y[40, 64] == 0.0
    assert np.array_equal(gr.clip_to_tile(X, 128), X)


def test_masks_against_loops():
    for M, N in [(1, 1), (33, 33), (130, 64), (300, 129), (257, 257)]:
        m = gr.mask_lower(M, N)
        for i in range(M):
            for j in range(N):
                assert m[i, j] == (j <= i)
    for M, nb, step, diag in gr.STAIR:
        blk = gr.STAIR_BLK
        m = gr.mask_stair(M, nb, blk, step, diag)
        assert m.shape == (M, nb * blk)
        for b in range(nb):
            for i in range(M):
                for c in range(blk):
                    r = i - b * step                     # row inside the block's own rows
                    want = r >= 0 and (not diag or c <= r)
                    assert m[i, b * blk + c] == want, (M, nb, step, diag, b, i, c)


def test_combine_leaves_c0_out_when_beta_is_zero():
    A, B, C0 = gr.scaled(17, 33, 16)
    bad = np.full_like(C0, np.nan)
    r0, s0 = gr.ref_nt(A, B, bad, -3.25, 0.0)
    r1, s1 = gr.ref_nt(A, B, None, -3.25, 0.0)
    assert np.array_equal(r0, r1) and np.array_equal(s0, s1) and np.all(np.isfinite(r0))
    m = gr.mask_lower(17, 33)
    r2, s2 = gr.ref_nt(A, B, C0, 0.37, -0.5, m)
    assert np.array_equal(r2[~m], gr.ld(C0)[~m]) and np.all(s2[~m] == 0) and np.all(s2[m] > 0)
