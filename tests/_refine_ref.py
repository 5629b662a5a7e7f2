"""
TEST INFRASTRUCTURE ONLY -- references, metrics, input builders and the case tables for the refinement step of the LML's
quadratic form (csrc/refine.hip, csrc/refine_tail.h).  Host only: nothing here touches the GPU.

What each kernel is held to (tests/test_gpu_refine_xref.py), and where the CPU side of it is tested (tests/test_refine_ref_host.py):

  back-substitution   a = L^-T alpha against tests/_xref.py's long-double substitution with the SAME (native) L and alpha, in a
                      metric that weighs row i by sqrt(A_ii) (a_i scales like 1 / sqrt(A_ii)); tolerance fr.tol(e64), e64 the
                      larger error of an fp64 model of the kernel's algorithm and of LAPACK (`backsub_e64`).
  residual pass       Kyy a in double-double: against the long-double product of the ASSEMBLED fp64 matrix with a, within that
                      product's own error bound n 2^-63 (|M| |a|)_i (`kyy_a_bound`).  A plain fp64 product misses that bound
                      (the negative control), so a double-double sum that lost its error terms would too.
  finish              quad = sum a_i (2 (y - m)_i - ka_i) in double-double.  Long double is no reference here: its own summation
                      error n 2^-64 S (S = sum |a_i t_i|) exceeds what double-double delivers as soon as the sum cancels -- and
                      the inputs are built to cancel (`cancelling_finish_inputs`: |quad| ~ 2^-22 S), because on data that does
                      not cancel a plain fp64 sum passes every tolerance one can justify.  The reference is exact rational
                      arithmetic (`finish_exact`); the tolerance max(16 |finish_model - exact|, 2 u |quad|) comes from a Python
                      statement of the kernel's double-double algorithm (`finish_model`), never from the kernel.

The double-double helpers restate csrc/refine_tail.h operation for operation in Python floats (IEEE binary64, every operation
rounded on its own); the product's rounding error is exact (math.fma, or fractions.Fraction where the interpreter lacks it).

gptorch_amd never imports this module.
"""
import math
from fractions import Fraction

import numpy as np
import torch

from gptorch_amd import rng
from tests import _factor_ref as fr
from tests import _xref as xr

LD = xr.LD
U = fr.U
LEAF = fr.LEAF
RT = 64                            # tile edge of the residual kernels (refine_tail.h)
VAR = 1.3
KIND_LIST = ("Rbf", "Matern52", "Matern32", "Exp", "Periodic")


# ---------------------------------------------------------------------------------------------------------------------
# planted points (shared with tests/test_gpu_kinds_xref.py and tests/test_gpu_expr_xref.py)
# ---------------------------------------------------------------------------------------------------------------------
def points(seed, n, d, ls0, first=0):
    """n random rows with the edges of the kernels planted (from row `first` on, spread over the tiles): exactly repeated
    rows, rows 1e-21 ell apart (r^2 = 1e-42, under the clamp), 1e-19 ell apart (r^2 = 1e-38, just above it), a row 1000 ell
    away (every exp underflows) and rows at r = pi/2 +- 1e-3, pi +- 1e-3 from the origin (Periodic's sign changes)."""
    x = rng.normal(seed, (n, d))
    e0 = np.zeros(d)
    e0[0] = ls0
    special = [np.zeros(d), 1e-21 * e0, 1e-19 * e0, None, 1000.0 * e0,
               (math.pi / 2 - 1e-3) * e0, (math.pi / 2 + 1e-3) * e0, (math.pi - 1e-3) * e0, (math.pi + 1e-3) * e0, np.zeros(d)]
    rows = [first + 7 * i for i in range(len(special))]
    for r, s in zip(rows, special):
        if r < n:
            x[r] = x[rows[0] + 1 if rows[0] + 1 < n else 0] if s is None else s
    return x


def length_scales(d, ard, seed, scale):
    """one length scale, or d of them spread over 0.6 .. 1.4 of `scale`"""
    return scale * (0.6 + 0.8 * rng.uniform(seed, d)) if ard else float(scale)


# ---------------------------------------------------------------------------------------------------------------------
# back-substitution
# ---------------------------------------------------------------------------------------------------------------------
def backsub_ref(L, alpha):
    """(L^-T alpha^T)^T [dy, n] in long double, alpha [dy, n] (the factor's extra rows)."""
    return xr.solve_upper_t(xr.ld(L), xr.ld(alpha).T).T


def backsub_metric(a, ref, sd):
    """max_i |a - a_ref|_i sqrt(A_ii) / max(1, max_i |a_ref|_i sqrt(A_ii)), in long double; a, ref [dy, n], sd = sqrt(A_ii) [n]."""
    a, ref, sd = xr.ld(a), xr.ld(ref), xr.ld(sd)
    if not ref.size:
        return 0.0
    return float(np.max(np.abs(a - ref) * sd[None, :]) / max(LD(1), np.max(np.abs(ref) * sd[None, :])))


def backsub_model64(L, alpha, nb=LEAF):
    """the kernel's algorithm in numpy fp64: column blocks of nb in descending order, s_j = alpha_j - sum_{k > j} L_kj^T a_k (k
    descending), a_j = W_j^T s_j with the EXPLICIT leaf inverse W_j = fr.lower_inverse64(L_jj).  alpha, result [dy, n]."""
    n = L.shape[0]
    alpha = np.asarray(alpha, dtype=np.float64)
    a = np.zeros_like(alpha)
    starts = list(range(0, n, nb))
    for c0 in reversed(starts):
        c1 = min(c0 + nb, n)
        s = alpha[:, c0:c1].copy()
        for k0 in reversed(starts):
            if k0 <= c0:
                break
            k1 = min(k0 + nb, n)
            s -= a[:, k0:k1] @ L[k0:k1, c0:c1]
        a[:, c0:c1] = s @ fr.lower_inverse64(np.ascontiguousarray(L[c0:c1, c0:c1]))
    return a


def row_scales(L):
    """sqrt(A_ii) of A = L L^T: the norms of L's rows"""
    return np.sqrt(np.sum(np.asarray(L, dtype=np.float64) ** 2, axis=1))


def backsub_e64(L, alpha, ref, sd=None):
    """e64 of the back-substitution against the long-double `ref` in `backsub_metric`: the larger of (a) backsub_model64's and
    (b) LAPACK's (torch.linalg.solve_triangular on the CPU) error -- the transposed counterpart of fr.solve_e64.
    sd: sqrt(A_ii) where the caller has the matrix (default: from L)."""
    L = np.ascontiguousarray(L, dtype=np.float64)
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    sd = row_scales(L) if sd is None else sd
    lap = torch.linalg.solve_triangular(torch.tensor(L).t(), torch.tensor(alpha.T.copy()), upper=True).numpy().T
    return max(backsub_metric(backsub_model64(L, alpha), ref, sd), backsub_metric(lap, ref, sd))


# (family, n) of the back-substitution table: `well` at every size where the code takes another path (n < 128, a full block, a
# ragged last block, several blocks), three families at three sizes; every one with dy = 1 (<1>), 2 (one <RDY> pass), 3 (a ragged
# second pass), 5 (three passes)
BACKSUB_SIZES = (1, 2, 127, 128, 129, 256, 257, 385, 641, 1100)
BACKSUB_FAMILIES_AT = (129, 385, 1100)
BACKSUB_DY = (1, 2, 3, 5)
BACKSUB_STEPWISE_N = (1, 127, 128, 129, 257)
BACKSUB_BATCHED = ((129, 3), (257, 1))


def backsub_cases():
    out = [("well", n) for n in BACKSUB_SIZES]
    out += [(fam, n) for n in BACKSUB_FAMILIES_AT for fam in ("graded10", "rbf_ill")]
    return [(fam, n, dy) for fam, n in out for dy in BACKSUB_DY]


# ---------------------------------------------------------------------------------------------------------------------
# double-double in Python floats: csrc/refine_tail.h, operation for operation
# ---------------------------------------------------------------------------------------------------------------------
if hasattr(math, "fma"):
    fma = math.fma
else:
    def fma(a, b, c):
        """a * b + c rounded once (float(Fraction) rounds to nearest even)"""
        return float(Fraction(a) * Fraction(b) + Fraction(c))


def two_sum(a, b):
    s = a + b
    bb = s - a
    e = (a - (s - bb)) + (b - bb)
    return s, e


def dd_fma(acc, a, b):
    """acc + a * b, acc = (hi, lo): error-free product and sum"""
    p = a * b
    ep = fma(a, b, -p)
    s, es = two_sum(acc[0], p)
    return s, acc[1] + (es + ep)


def dd_add(acc, x):
    s, e = two_sum(acc[0], x[0])
    return s, acc[1] + (e + x[1])


def _residual(y, m, i, c):
    """(y - m)_ic rounded once (as in the extra rows the factorisation consumed)"""
    return float(y[i, c]) - float(m[i, c]) if m is not None else float(y[i, c])


def finish_model(y, m, a, ka_hi, ka_lo):
    """refine_finish_kernel's algorithm in one fixed order (right-hand side by right-hand side, row by row): per entry
    t = 2 (y - m) - ka as a double-double with (y - m) rounded once, q += a_i t.hi error-free, q.lo += a_i t.lo; -> q.hi + q.lo.
    y, m [n, dy] (m None: no mean); a, ka_hi, ka_lo [dy, n]."""
    n, dy = y.shape
    q = (0.0, 0.0)
    for c in range(dy):
        for i in range(n):
            ka = dd_add((0.0, 0.0), (float(ka_hi[c, i]), float(ka_lo[c, i])))
            r = _residual(y, m, i, c)
            t = dd_add((0.0, 0.0), (-ka[0], -ka[1]))
            t = dd_add(t, (r, 0.0))
            t = dd_add(t, (r, 0.0))
            ai = float(a[c, i])
            q = dd_fma(q, ai, t[0])
            q = (q[0], fma(ai, t[1], q[1]))
    return q[0] + q[1]


def finish_exact(y, m, a, ka_hi, ka_lo):
    """-> (quad, S) as Fractions: quad = sum a_i (2 (y - m)_i - ka_hi_i - ka_lo_i) from the same fp64 inputs ((y - m) rounded once)
    without any further rounding, S = sum |a_i t_i|."""
    n, dy = y.shape
    quad, S = Fraction(0), Fraction(0)
    for c in range(dy):
        for i in range(n):
            t = 2 * Fraction(_residual(y, m, i, c)) - Fraction(float(ka_hi[c, i])) - Fraction(float(ka_lo[c, i]))
            p = Fraction(float(a[c, i])) * t
            quad += p
            S += abs(p)
    return quad, S


def finish_fp64(y, m, a, ka_hi, ka_lo):
    """the negative control: the same quantity as a plain fp64 expression"""
    r = (y - m) if m is not None else y
    return float(np.sum(a * (2 * r.T - ka_hi - ka_lo)))


def finish_tol(model, quad):
    """max(16 |finish_model - exact|, 2 u |quad_exact|): sixteen times the error of a CPU statement of the same algorithm, floored
    at two roundings of the result"""
    return max(16.0 * abs(float(Fraction(model) - quad)), 2 * U * abs(float(quad)))


def frac_err(x, exact):
    """|x - exact| for an fp64 x and a Fraction, formed exactly and rounded once"""
    return abs(float(Fraction(float(x)) - exact))


def lml_term(sum_log, quad, n, dy):
    """-1/2 quad - dy sum_log - 1/2 dy n log 2 pi in long double, and the size of its largest term"""
    t = (LD(0.5) * LD(quad), LD(dy) * LD(sum_log), LD(0.5) * dy * n * np.log(2 * LD(np.pi)))
    return -t[0] - t[1] - t[2], float(max(abs(v) for v in t))


# n: 1024 and 1025 sit either side of one element per thread of the single 1024-thread workgroup
FINISH_CASES = [(n, dy, with_m) for n in (1, 65, 1024, 1025, 1100) for dy in (1, 3) for with_m in (True, False)]
FINISH_CONTROL_MISS = 100.0


def cancelling_finish_inputs(n, dy, seed):
    """-> y, m [n, dy], a, ka_hi, ka_lo [dy, n] as they stand after a real step: ka = Kyy a_hat within 1e-9 of (y - m), a
    normalised double-double (|lo| <= 2^-54 |hi|); and a sum that CANCELS: the last (up to three) entries of a are solved so
    that quad = sum a_i t_i is 2^-22 of the sum of the other entries' |a_i t_i|, i.e. 2^-23 .. 2^-22 of S.  A single term
    (n dy = 1) cannot cancel: it is returned as drawn."""
    y = rng.normal(8100 + seed, (n, dy))
    m = 0.3 * rng.normal(8200 + seed, (n, dy))
    r = (y - m).T                                                # [dy, n], rounded once
    ka_hi = r * (1.0 + 1e-9 * rng.normal(8300 + seed, (dy, n)))
    ka_lo = ka_hi * 2.0 ** -54 * (2.0 * rng.uniform(8400 + seed, dy * n).reshape(dy, n) - 1.0)
    a = rng.normal(8500 + seed, (dy, n))
    N = n * dy
    k = min(3, N - 1)
    if k > 0:
        flat = [(c, i) for c in range(dy) for i in range(n)]
        t = {ci: 2 * Fraction(float(r[ci])) - Fraction(float(ka_hi[ci])) - Fraction(float(ka_lo[ci])) for ci in flat[N - k:]}
        P, S = Fraction(0), Fraction(0)
        for c, i in flat[:N - k]:
            p = Fraction(float(a[c, i])) * (2 * Fraction(float(r[c, i])) - Fraction(float(ka_hi[c, i])) - Fraction(float(ka_lo[c, i])))
            P += p
            S += abs(p)
        want = S / 2 ** 22
        for j, ci in enumerate(flat[N - k:]):
            share = (want - P) / (k - j)                        # the last entry takes all that is left
            a[ci] = float(share / t[ci])
            P += Fraction(float(a[ci])) * t[ci]
    return y, m, a, ka_hi, ka_lo


# ---------------------------------------------------------------------------------------------------------------------
# residual pass
# ---------------------------------------------------------------------------------------------------------------------
def kyy_a_bound(M, a):
    """n 2^-63 (|M| |a|)_i in long double, [dy, n] for a [dy, n]: the error bound of the long-double product M a itself
    (n 2^-64 |M| |a|), with a factor of two."""
    M, a = xr.ld(M), xr.ld(a)
    n = M.shape[0]
    return n * LD(2) ** -63 * (np.abs(a) @ np.abs(M).T)


def product_ld(M, a):
    """(M a^T)^T [dy, n] in long double from fp64 M [n, n] and a [dy, n]"""
    return xr.ld(a) @ xr.ld(M).T


def product_sequential64(M, a):
    """the same product in fp64, one column of M after the other: acc_i += M_ij a_j for j = 0, 1, ..."""
    M, a = np.asarray(M, dtype=np.float64), np.asarray(a, dtype=np.float64)
    out = np.zeros((a.shape[0], M.shape[0]))
    for c in range(a.shape[0]):
        acc = np.zeros(M.shape[0])
        for j in range(M.shape[1]):
            acc = acc + M[:, j] * a[c, j]
        out[c] = acc
    return out


def fp64_product_misses(M, a):
    """the negative control of the residual pass: max over rows of |fp64 product - long-double product| / kyy_a_bound, for numpy's
    product and the sequential one -> (numpy's, sequential).  Rows whose bound is zero (a zero row of |M| |a|) are exact in every
    arithmetic and left out."""
    exact, bound = product_ld(M, a), kyy_a_bound(M, a)
    keep = bound > 0
    out = []
    for got in (np.asarray(a, dtype=np.float64) @ np.asarray(M, dtype=np.float64).T, product_sequential64(M, a)):
        out.append(float(np.max(np.abs(xr.ld(got) - exact)[keep] / bound[keep])))
    return tuple(out)


RESID_SHAPES = [(1, 1, False), (63, 3, True), (64, 16, False), (65, 17, True), (130, 2, False), (257, 33, True)]   # 17, 33: past the 16-coordinate staging pass
RESID_DY = (1, 2, 3)
RESID_NOISE = 0.07


def resid_cases():
    """(kind, n, d, ard, dy): every kind with every shape, dy dealt round so that every kind and every shape meets every dy"""
    return [(kind, n, d, ard, RESID_DY[(i + j) % 3]) for i, kind in enumerate(KIND_LIST) for j, (n, d, ard) in enumerate(RESID_SHAPES)]


def resid_inputs(kind, n, d, ard, dy):
    """-> points [n, d] with the kernels' edges planted, length scale(s), a [dy, n]"""
    ls = length_scales(d, ard, 40 + d, 0.8 * math.sqrt(d))
    xn = points(n + 7 * d + KIND_LIST.index(kind), n, d, float(np.atleast_1d(ls)[0]))
    a = rng.normal(900 + n + dy + 10 * KIND_LIST.index(kind), (dy, n))
    return xn, ls, a


def kyy64(kind, xn, ls, noise, variance=VAR):
    """Kyy in plain fp64 on the CPU (direct differences): the stand-in for the assembled matrix where no GPU is at hand"""
    K = xr.direct_kernel_K(kind, torch.tensor(xn), None, torch.tensor([variance], dtype=torch.float64),
                           torch.tensor(np.atleast_1d(np.asarray(ls, dtype=np.float64)))).numpy().copy()
    K[np.arange(len(xn)), np.arange(len(xn))] += noise
    return K


# ---------------------------------------------------------------------------------------------------------------------
# the composed step at small sizes
# ---------------------------------------------------------------------------------------------------------------------
# (kind, n, d, dy, ard, mean, noise); the last: noise 1e-4, so that the factor's error is visible in the plain value
STEP_CASES = [("Rbf", 1, 1, 1, False, False, 0.05), ("Matern52", 64, 3, 2, True, True, 0.05), ("Exp", 65, 2, 3, False, True, 0.05),
              ("Periodic", 128, 1, 1, False, False, 0.05), ("Matern32", 129, 17, 2, True, True, 0.05), ("Rbf", 257, 4, 5, False, False, 1e-4)]


def step_inputs(kind, n, d, dy, ard, mean, noise):
    """-> x [n, d], y [n, dy], length scale(s), mean [dy] or None"""
    x, y = rng.make_regression(n, d, dy, seed=n + d)
    ls = length_scales(d, ard, 70 + d, 1.5 if d == 1 else 0.9 * math.sqrt(d))
    return x, y, ls, (np.linspace(-0.3, 0.25, dy) if mean else None)


def _ints(x):
    """fp64 array -> (object array of Python ints, e) with x = ints * 2^e exactly"""
    x = np.asarray(x, dtype=np.float64)
    mant, ex = np.frexp(x)
    mant = (mant * 2.0 ** 53).astype(np.int64)                  # exact: |mant| < 2^53
    ex = ex.astype(np.int64) - 53
    nz = mant != 0
    e0 = int(ex[nz].min()) if nz.any() else 0
    out = np.empty(x.shape, dtype=object)
    for idx in np.ndindex(x.shape):
        out[idx] = int(mant[idx]) << int(ex[idx] - e0) if mant[idx] else 0
    return out, e0


def step_quad_exact(r, M, a):
    """sum_c sum_i a_ci (2 r_ci - (M a_c)_i) in exact (dyadic rational) arithmetic from fp64 r [dy, n], M [n, n], a [dy, n]
    -> Fraction.  (Integers at a common binary exponent instead of fractions.Fraction per entry: n^2 dy products.)"""
    Ri, er = _ints(r)
    Mi, em = _ints(M)
    Ai, ea = _ints(a)
    MA = Ai.dot(Mi.T)                                            # exponent em + ea
    e0 = min(er + 1, em + ea)
    total = 0
    for c in range(Ai.shape[0]):
        for i in range(Ai.shape[1]):
            t = (int(Ri[c, i]) << (er + 1 - e0)) - (int(MA[c, i]) << (em + ea - e0))
            total += int(Ai[c, i]) * t
    return Fraction(total) * Fraction(2) ** (e0 + ea)


# ---------------------------------------------------------------------------------------------------------------------
# gemv_t
# ---------------------------------------------------------------------------------------------------------------------
GEMV_SHAPES = [(1, 1), (31, 255), (32, 256), (33, 257), (256, 700), (257, 64), (1000, 129)]
GEMV_DY = (1, 2, 3)


def gemv_inputs(rows, cols, dy):
    """-> L [rows, cols], a [dy, rows], c0 [dy, cols] (non-zero: the entry point accumulates)"""
    s = 9000 + 7 * rows + cols + dy
    return rng.normal(s, (rows, cols)), rng.normal(s + 1, (dy, rows)), rng.normal(s + 2, (dy, cols))


def gemv_metric(c, L, a, c0):
    """max_j |c - (c0 + L^T a)|_j / (|c0|_j + (|L|^T |a|)_j), the reference in long double; c, c0 [dy, cols]"""
    ref = xr.ld(c0) + xr.ld(a) @ xr.ld(L)
    scale = np.abs(xr.ld(c0)) + np.abs(xr.ld(a)) @ np.abs(xr.ld(L))
    return float(np.max(np.abs(xr.ld(c) - ref) / scale))
