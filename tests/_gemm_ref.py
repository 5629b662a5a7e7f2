"""
TEST INFRASTRUCTURE ONLY -- data, masks, a long-double reference and the a-priori bound for the fp64 "NT" contraction
C = alpha A B^T + beta C0 (csrc/gemm_f64.hip, csrc/gemm_tile.h).  Host only: nothing here touches the GPU.

Reference: the same statement in np.longdouble (64-bit mantissa here: K 2^-64 S of error, 1/2048 of the bound below;
tests/test_gemm_ref_host.py holds it to exact rational arithmetic).  Every comparison is ENTRYWISE against

    bound(K, S) = (K + 3) 2^-53 S,     S = |alpha| |A| |B|^T + |beta| |C0|     (entry by entry)

the textbook bound for K rounded products, K - 1 additions in ANY order, the rounding of alpha * acc and the final fma (fused
MFMA accumulation only removes roundings).  It is derived from the operation count, not tuned against the kernel; numpy's own
fp64 product is checked to stay inside it on every family and shape used on the GPU (test_gemm_ref_host.py), so it is never
tighter than a correct fp64 product needs.  Where products or sums fall below 2^-1022 every one of those K + 2 operations can
lose another 2^-1075 absolutely (gradual underflow): `tiny` = K 2^-1074 covers them.

gptorch_amd never imports this module.
"""
import functools

import numpy as np

from gptorch_amd import rng

LD = np.longdouble
U = 2.0 ** -53
SENTINEL = -7.25                       # what entries that a launch must not write hold before it

TRI_A_UPPER, TRI_A_LOWER, TRI_B_UPPER, TRI_B_LOWER = 1, 2, 4, 8

# ---------------------------------------------------------------------------------------------------------------------
# what the GPU module runs (tests/test_gemm_ref_host.py walks the same lists)
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1, 16), (16, 16, 16), (17, 33, 16), (31, 129, 48), (65, 63, 80), (129, 127, 144), (200, 72, 272), (257, 130, 528))
VARIANTS = (0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11)          # gpn_debug_set_gemm_variant: 0 the shipped dispatch, 1 register staging,
TILE_EDGE = {3: 128, 4: 64, 5: 64, 6: 32, 7: 128, 8: 64, 9: 128, 10: 128, 11: 128}     # 3..11 forced tile shapes (BM = BN)
SHIPPED = (6, 8, 11)                                    # the three shapes the shipped dispatch picks from
PAIRS = ((1.0, 0.0), (-1.0, 1.0), (0.37, -0.5), (2.0 ** -30, 1.0), (-3.25, 0.0))       # (alpha, beta)
FAMILIES = ("scaled", "cancel", "tiny", "tri")
LOWER1 = tuple((n, K) for n in (1, 33, 130, 257) for K in (16, 80))
LOWER2 = ((130, 64, 48), (300, 129, 48), (257, 257, 48))                               # (M, N, K)
STAIR_BLK, STAIR_K = 128, 48
STAIR = ((300, 2, 128, 1), (520, 3, 256, 0), (400, 3, 0, 1), (260, 3, 128, 0))         # (M, nb, step, diag)
TRI_SHAPES = ((200, 72, 208), (72, 200, 208), (300, 130, 144))                         # the last: M > K
THIN_SHAPES = ((1, 130, 64), (16, 64, 32), (129, 65, 48), (145, 33, 80))
BATCH_SHAPE = (200, 200, 48)           # one problem: 32 x 32 tiles; five of them: 64 x 64 (gemm_nt_impl's tiles(b) * batch)
SPLITK = (130, 72, 48, 5)              # (M, N, K of one part, parts)
MATMUL_K = (1, 17, 50)


def round_up(n, m):
    return (n + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------------------------
# reference and bound
# ---------------------------------------------------------------------------------------------------------------------
def ld(a):
    return np.asarray(a, dtype=LD)


def product_ld(A, B):
    """(A B^T, |A| |B|^T) as long doubles.  The product itself is formed in long double.  The scale has only positive terms, so
    an fp64 BLAS product of the operands scaled to O(1) by exact powers of two (nothing underflows on `tiny`) is within
    K 2^-53 of it; it is inflated by (K + 2) 2^-52 so that it never comes out below the true scale."""
    a, b = ld(A), ld(B)
    K = A.shape[1]
    sa, sb = (-int(np.frexp(np.abs(X).max())[1]) if np.abs(X).max() > 0 else 0 for X in (A, B))
    SP = np.abs(np.ldexp(A, sa)) @ np.abs(np.ldexp(B, sb)).T
    return a @ b.T, np.ldexp(ld(SP) * (1 + LD(K + 2) * LD(2.0) ** -52), -(sa + sb))


def combine(P, SP, C0, alpha, beta, mask=None):
    """reference and scale from the long-double product: entries outside `mask` keep C0 (and have scale 0)"""
    ref, S = LD(alpha) * P, abs(LD(alpha)) * SP
    if beta != 0.0:                    # beta == 0: C0 is not an input at all (it may hold NaN)
        ref = ref + LD(beta) * ld(C0)
        S = S + abs(LD(beta)) * np.abs(ld(C0))
    if mask is not None:
        ref = np.where(mask, ref, ld(C0))
        S = np.where(mask, S, LD(0))
    return ref, S


def ref_nt(A, B, C0=None, alpha=1.0, beta=0.0, mask=None):
    """-> (alpha A B^T + beta C0, S = |alpha| |A| |B|^T + |beta| |C0|), both long double [M, N]"""
    P, SP = product_ld(A, B)
    return combine(P, SP, C0, alpha, beta, mask)


def bound(K, S, tiny=0.0):
    return LD(K + 3) * LD(U) * S + LD(tiny)


def tiny_of(family, K):
    return K * 2.0 ** -1074 if family == "tiny" else 0.0


def units(got, ref, S, K=0, tiny=0.0):
    """worst |got - ref| / (2^-53 S) over the entries with S > 0 (with `tiny`: / (2^-53 S + tiny / (K + 3)), the bound's unit)"""
    err = np.abs(ld(got) - ref)
    ok = S > 0
    return float(np.max(err[ok] / (LD(U) * S[ok] + LD(tiny) / (K + 3)))) if ok.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# masks: True where a launch writes
# ---------------------------------------------------------------------------------------------------------------------
def mask_lower(M, N):
    """lower = 1 (M == N) and lower = 2 (trapezoid, M >= N): the entries with j <= i"""
    return np.arange(N)[None, :] <= np.arange(M)[:, None]


def mask_stair(M, nb, blk, step, diag):
    """gpn_gemm_nt_stair: column block b has the rows from b * step on; with diag its first blk x blk square is lower-only"""
    rows, cols = np.arange(M)[:, None], np.arange(nb * blk)[None, :]
    start = (cols // blk) * step
    keep = rows >= start
    if diag:
        keep = keep & ((cols % blk) <= (rows - start))
    return keep


# ---------------------------------------------------------------------------------------------------------------------
# data families (gptorch_amd.rng: the same bits everywhere), full 53-bit mantissas
# ---------------------------------------------------------------------------------------------------------------------
def _seed(family, M, N, K, salt=0):
    return 9000 + 1000003 * FAMILIES.index(family) + 7919 * M + 104729 * N + 31 * K + 15485863 * salt


def _exponents(seed, n):
    """integers uniform in [-40, 40]"""
    return np.floor(rng.uniform(seed, n) * 81.0).astype(np.int64) - 40


def scaled(M, N, K, salt=0, shift=0):
    """randn with row i of A times 2^e_i, row j of B times 2^f_j, C0 randn times 2^(e_i + f_j): every entry of C has its own
    scale, spread over 2^+-80 (a normwise check would hide every small one).  shift: both operands times 2^shift."""
    s = _seed("scaled", M, N, K, salt)
    e, f = _exponents(s + 3, M), _exponents(s + 4, N)
    A = np.ldexp(rng.normal(s, (M, K)), (e + shift)[:, None])
    B = np.ldexp(rng.normal(s + 1, (N, K)), (f + shift)[:, None])
    C0 = np.ldexp(rng.normal(s + 2, (M, N)) * np.sqrt(K), e[:, None] + f[None, :] + 2 * shift)
    return A, B, C0


def tiny(M, N, K, salt=0):
    """`scaled` times 2^-520 per operand: the products lie around 2^-1040 2^+-80, most of them subnormal or below"""
    return scaled(M, N, K, salt + 1, shift=-520)


def cancel(M, N, K, salt=0):
    """columns in pairs, A[:, 2t+1] = A[:, 2t] and B[:, 2t+1] = -B[:, 2t] (1 + delta_t), delta ~ 1e-10: S / |C| ~ 1e10"""
    assert K % 2 == 0
    s = _seed("cancel", M, N, K, salt)
    A, B = np.empty((M, K)), np.empty((N, K))
    A[:, 0::2] = rng.normal(s, (M, K // 2))
    A[:, 1::2] = A[:, 0::2]
    B[:, 0::2] = rng.normal(s + 1, (N, K // 2))
    delta = 1e-10 * (1.0 + rng.uniform(s + 3, K // 2))
    B[:, 1::2] = -B[:, 0::2] * (1.0 + delta)[None, :]
    C0 = 1e-10 * np.sqrt(K) * rng.normal(s + 2, (M, N))
    return A, B, C0


def tri(M, N, K, flags, salt=0):
    """randn operands with the strict triangles of `flags` (GPN_TRI_*): A_UPPER A[i, k] = 0 for k < i, A_LOWER for k > i, and the
    same for B with its row index j"""
    s = _seed("tri", M, N, K, salt)
    A, B, C0 = rng.normal(s, (M, K)), rng.normal(s + 1, (N, K)), rng.normal(s + 2, (M, N))
    k = np.arange(K)[None, :]
    for X, rows, up, lo in ((A, M, TRI_A_UPPER, TRI_A_LOWER), (B, N, TRI_B_UPPER, TRI_B_LOWER)):
        r = np.arange(rows)[:, None]
        if flags & up:
            X[k < r] = 0.0
        if flags & lo:
            X[k > r] = 0.0
    return A, B, C0


def dense_to_edge(M, K, edge=128, salt=0):
    """an A_LOWER / B_LOWER operand that is NOT a triangle: row i dense up to the next multiple of `edge` after i"""
    X = rng.normal(_seed("tri", M, M, K, salt + 7), (M, K))
    X[np.arange(K)[None, :] >= (np.arange(M)[:, None] // edge + 1) * edge] = 0.0
    return X


def clip_to_tile(X, b):
    """what a launch with b x b tiles reads of an X_LOWER operand: row i up to k < b * (i // b + 1)"""
    Y = X.copy()
    Y[np.arange(X.shape[1])[None, :] >= (np.arange(X.shape[0])[:, None] // b + 1) * b] = 0.0
    return Y


def family(name, M, N, K, salt=0):
    """(A, B, C0) of a family; "tri" here is the U U^T-like pair (A_UPPER | B_UPPER), the flag sweep calls tri() itself"""
    if name == "tri":
        return tri(M, N, K, TRI_A_UPPER | TRI_B_UPPER, salt)
    return {"scaled": scaled, "cancel": cancel, "tiny": tiny}[name](M, N, K, salt)


@functools.lru_cache(maxsize=None)
def case(name, M, N, K, salt=0):
    """-> (A, B, C0, P, SP): a family's data with its long-double product and scale, computed once and shared (read only)"""
    A, B, C0 = family(name, M, N, K, salt)
    P, SP = product_ld(A, B)
    for x in (A, B, C0, P, SP):
        x.setflags(write=False)
    return A, B, C0, P, SP


@functools.lru_cache(maxsize=None)
def tri_case(M, N, K, flags):
    """-> (A, B, C0, P, SP) of tri(M, N, K, flags), shared like case()"""
    A, B, C0 = tri(M, N, K, flags)
    P, SP = product_ld(A, B)
    for x in (A, B, C0, P, SP):
        x.setflags(write=False)
    return A, B, C0, P, SP


def pair_of(*idx):
    """deal the (alpha, beta) pairs over the cases"""
    return PAIRS[sum(idx) % len(PAIRS)]
