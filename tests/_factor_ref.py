"""
TEST INFRASTRUCTURE ONLY -- matrices, an fp64 model and scale-aware metrics for the dense linear algebra under every model
(csrc/potrf.hip, leaf16*.h, colpanel.hip, trisolve.hip, ppotrf.hip).  Host only: nothing here touches the GPU.

The reference is tests/_xref.py's long-double Cholesky and substitutions.  A check of a native kernel is held to

    tol = max(16 e64, 8 * 2^-53)

where e64 is the error, in the SAME metric against the SAME long-double value, of a plain fp64 statement of the quantity --
the larger of
  * `model_factor`: the algorithm the kernels implement, in numpy fp64: right-looking in 128-column blocks, the diagonal block
    factored, W = L_kk^-1 formed explicitly, panel = B W^T, trailing update, the extra rows carried through the same solves;
  * LAPACK (torch.linalg.cholesky / solve_triangular on the CPU).
LAPACK alone is not a fair yardstick: multiplying by explicit leaf inverses costs a factor that grows with the leaf's condition
number (on kernel matrices with noise 1e-6 the model's scaled residual is 17-48 x LAPACK's), while on well-conditioned and
graded matrices the two agree within 2 u.  e64 is computed at test time on the CPU, never from GPU output.

Metrics are scale-aware (a row of scale 2^-60 counts like a row of scale 1) and formed in long double:
    forward    max |L - L_ref|_ij / sqrt(a_ii)
    residual   max_{i >= j} |L L^T - A|_ij / sqrt(a_ii a_jj)
    leaf       max |W_k L_ref,kk - I|
The residual is not formed as a long-double product (6 s at n = 1100).  With D = L - L_ref in long double,
    L L^T - A = D L_ref^T + L_ref D^T + D D^T + (L_ref L_ref^T - A),
and the last term is the long-double reference's own residual (n 2^-64 at most, a few 1e-3 u here: reported by
`FactorRef.ref_residual` on a sample and far below the 8 u floor).  D (rounded to fp64: a relative 2^-53 of an error) and L_ref
(rounded to fp64: 2^-53 relative, times D) are multiplied by fp64 BLAS after the rows are scaled by 2^round(-log2 sqrt(a_ii)),
which is exact; the BLAS rounding is n 2^-53 |D| |L|, i.e. a relative 1e-13 of the residual being measured.

gptorch_amd never imports this module.
"""
import numpy as np
import torch

from gptorch_amd import rng
from tests import _xref as xr

LD = np.longdouble
U = 2.0 ** -53
LEAF = 128
SAFETY = 16.0
FLOOR = 8 * U
FAMILIES = ("well", "graded2", "graded10", "rbf_ill")


def tol(e64):
    return max(SAFETY * e64, FLOOR)


# ---------------------------------------------------------------------------------------------------------------------
# matrix families (fp64 numpy, exactly symmetric)
# ---------------------------------------------------------------------------------------------------------------------
def _sym(A):
    L = np.tril(A)
    return L + np.tril(L, -1).T


def well(n, seed=0):
    """G G^T / n + 0.5 I: condition number ~ 10, every pivot >= 0.5."""
    G = rng.normal(7100 + seed, (n, n))
    return _sym(G @ G.T / n + 0.5 * np.eye(n))


def graded2_exponents(n, seed=0):
    """k_i integer, uniform in [-60, 60]"""
    return np.floor(rng.uniform(7200 + seed, n) * 121.0).astype(np.int64) - 60


def graded2(n, seed=0):
    """D well D with D = diag(2^k_i): the scaling is exact in fp64."""
    d = np.ldexp(1.0, graded2_exponents(n, seed))
    return well(n, seed) * d[:, None] * d[None, :]


def graded10(n, seed=0):
    """D well D with D = diag(10^U(-4, 4))"""
    d = 10.0 ** (8.0 * rng.uniform(7300 + seed, n) - 4.0)
    return _sym(well(n, seed) * d[:, None] * d[None, :])


def rbf_ill(n, seed=0):
    """exp(-r^2 / 8) on N(0, I_2) points + 1e-6 I: condition number ~ 3e8, the project's "ill" regime."""
    x = rng.normal(7400 + seed, (n, 2))
    r2 = (x[:, 0:1] - x[None, :, 0]) ** 2 + (x[:, 1:2] - x[None, :, 1]) ** 2
    return _sym(np.exp(-r2 / 8.0) + 1e-6 * np.eye(n))


def matrix(family, n, seed=0):
    return {"well": well, "graded2": graded2, "graded10": graded10, "rbf_ill": rbf_ill}[family](n, seed)


def rhs(A, e, seed=0):
    """[n, e] right-hand sides diag(sqrt(a_ii)) N(0, 1): the extra rows (L^-1 R)^T are O(1) whatever the row scales."""
    n = A.shape[0]
    return np.sqrt(np.diag(A))[:, None] * rng.normal(7500 + seed, (n, max(e, 1)))[:, :e]


def triangular(n, seed=0):
    """a lower-triangular matrix that is NOT a Cholesky factor: tril(N(0,1)) / sqrt(n), diagonal +-(1 + U(0,1)) of mixed sign"""
    T = np.tril(rng.normal(7600 + seed, (n, n)), -1) / np.sqrt(n)
    u = rng.uniform(7700 + seed, 2 * n)
    T[np.arange(n), np.arange(n)] = np.where(u[:n] < 0.5, -1.0, 1.0) * (1.0 + u[n:])
    if n > 1:
        T[0, 0], T[1, 1] = abs(T[0, 0]), -abs(T[1, 1])          # both signs, whatever the draw
    return T


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 model of the kernels' algorithm
# ---------------------------------------------------------------------------------------------------------------------
def lower_inverse64(L):
    """L^-1 by forward substitution on the identity, row by row (fp64)."""
    n = L.shape[0]
    W = np.zeros((n, n))
    for i in range(n):
        W[i, :i] = -(L[i, :i] @ W[:i, :i])
        W[i, i] = 1.0
        W[i, :i + 1] /= L[i, i]
    return W


def model_factor(A, R=None, nb=LEAF):
    """-> (L [n, n], extra [e, n] = (L^-1 R)^T, winv [nblocks, nb, nb]) in fp64, by the kernels' algorithm (module docstring)."""
    n = A.shape[0]
    e = 0 if R is None else R.shape[1]
    M = np.zeros((n + e, n))
    M[:n] = np.tril(A)
    if e:
        M[n:] = R.T
    W = np.zeros(((n + nb - 1) // nb, nb, nb))
    for b, k in enumerate(range(0, n, nb)):
        c = min(k + nb, n)
        Lkk = np.linalg.cholesky(_sym(M[k:c, k:c]))
        M[k:c, k:c] = Lkk
        W[b, :c - k, :c - k] = lower_inverse64(Lkk)
        if c < n + e:
            M[c:, k:c] = M[c:, k:c] @ W[b, :c - k, :c - k].T
        if c < n:
            P = M[c:, k:c]
            M[c:n, c:] -= np.tril(P[:n - c] @ P[:n - c].T)
            if e:
                M[n:, c:] -= P[n - c:] @ P[:n - c].T
    return np.tril(M[:n]), M[n:].copy(), W


def model_solve(L, B, nb=LEAF):
    """L^-1 B in fp64 the way the native right-solves do it: block forward substitution with the EXPLICIT inverses of the nb x nb
    diagonal blocks (X_k = W_k (B_k - sum_{j<k} L_kj X_j))."""
    n = L.shape[0]
    X = np.array(B, dtype=np.float64)
    for k in range(0, n, nb):
        c = min(k + nb, n)
        X[k:c] = lower_inverse64(L[k:c, k:c]) @ (X[k:c] - L[k:c, :k] @ X[:k])
    return X


def solve_e64(L, B, ref, nb=LEAF):
    """e64 of a triangular solve L^-1 B against the long-double `ref`: the larger of model_solve's (explicit inverses of the
    nb x nb diagonal blocks) and LAPACK's error"""
    lap = torch.linalg.solve_triangular(torch.tensor(L), torch.tensor(np.ascontiguousarray(B)), upper=False).numpy()
    return max(xr.abs_err(model_solve(L, B, nb), ref), xr.abs_err(lap, ref))


def lapack_factor(A, R=None):
    """torch's CPU Cholesky and triangular solve: (L, extra [e, n], winv [nblocks, 128, 128] from solve_triangular)"""
    n = A.shape[0]
    L = torch.linalg.cholesky(torch.tensor(A))
    E = np.zeros((0, n))
    if R is not None and R.shape[1]:
        E = torch.linalg.solve_triangular(L, torch.tensor(R), upper=False).t().contiguous().numpy()
    W = np.zeros(((n + LEAF - 1) // LEAF, LEAF, LEAF))
    for b, k in enumerate(range(0, n, LEAF)):
        c = min(k + LEAF, n)
        W[b, :c - k, :c - k] = torch.linalg.solve_triangular(L[k:c, k:c], torch.eye(c - k, dtype=torch.float64), upper=False).numpy()
    return L.numpy(), E, W


# ---------------------------------------------------------------------------------------------------------------------
# long-double reference of one (matrix, right-hand sides) and the metrics against it
# ---------------------------------------------------------------------------------------------------------------------
class FactorRef:
    """long-double factor, extra rows and LML terms of A (fp64 numpy) with right-hand sides R [n, e]; the metrics; and e64 per
    metric (the larger of the fp64 model's and LAPACK's error)."""

    def __init__(self, A, R=None):
        self.A = A
        self.n = n = A.shape[0]
        self.e = 0 if R is None else R.shape[1]
        self.R = R
        self.L = xr.cholesky(A)                                  # raises if A is not positive definite in long double
        self.sd = np.sqrt(xr.ld(np.diag(A)))                    # sqrt(a_ii)
        self.extra_ref = xr.solve_lower(self.L, R).T if self.e else np.zeros((0, n), dtype=LD)
        self.logdiag = np.log(np.diag(self.L))
        self.sumsq = np.sum(self.extra_ref ** 2)
        self.lml_ref = (np.sum(self.logdiag), self.sumsq,
                        -LD(0.5) * self.sumsq - self.e * np.sum(self.logdiag) - LD(0.5) * self.e * n * np.log(2 * LD(np.pi)))
        # row scales as exact powers of two for the fp64 products of `residual`
        self._p2 = np.ldexp(1.0, -np.round(np.log2(self.sd.astype(np.float64))).astype(np.int64))
        self._Ls = (self.L * self._p2[:, None]).astype(np.float64)
        self._ratio = (self.sd * self._p2).astype(np.float64)   # sqrt(a_ii) 2^-round(log2 sqrt(a_ii)) in [0.7, 1.42]
        self.e64 = {}
        fm, fl = model_factor(A, R), lapack_factor(A, R)
        for what, fn in (("forward", self.forward), ("residual", self.residual)):
            self.e64[what] = max(fn(fm[0]), fn(fl[0]))
        self.e64["extra"] = max(self.extra_err(fm[1]), self.extra_err(fl[1])) if self.e else 0.0
        self.e64["leaf"] = [max(a, b) for a, b in zip(self.leaf_errs(fm[2]), self.leaf_errs(fl[2]))]
        lm, ll = self.lml64(fm[0], fm[1]), self.lml64(fl[0], fl[1])
        self.e64["lml"] = [max(abs(float(LD(a) - r)), abs(float(LD(b) - r))) for a, b, r in zip(lm, ll, self.lml_ref)]

    def forward(self, L):
        return float(np.max(np.abs(np.tril(xr.ld(L)) - self.L) / self.sd[:, None]))

    def residual(self, L):
        D = ((np.tril(xr.ld(L)) - self.L) * self._p2[:, None]).astype(np.float64)
        T = D @ self._Ls.T
        Rm = np.tril(T + T.T + D @ D.T) / self._ratio[:, None] / self._ratio[None, :]
        return float(np.max(np.abs(Rm)))

    def ref_residual(self, rows=64):
        """the long-double reference's own scaled residual on the last `rows` rows (what `residual` leaves out)"""
        i0 = max(0, self.n - rows)
        P = np.einsum("ik,jk->ij", self.L[i0:], self.L) - xr.ld(self.A[i0:])
        return float(np.max(np.abs(np.tril(P, i0)) / self.sd[i0:, None] / self.sd[None, :]))

    def extra_err(self, E):
        return xr.abs_err(E, self.extra_ref)

    def leaf_errs(self, W):
        """per 128-block k: max |W_k L_ref,kk - I| over the kb x kb block"""
        out = []
        W = xr.ld(W).reshape(-1, LEAF, LEAF)
        for b, k in enumerate(range(0, self.n, LEAF)):
            c = min(k + LEAF, self.n)
            P = np.einsum("ik,kj->ij", W[b, :c - k, :c - k], self.L[k:c, k:c])
            out.append(float(np.max(np.abs(P - np.eye(c - k, dtype=LD)))))
        return out

    @staticmethod
    def lml64(L, E):
        """the three terms of gpn_lml_reduce from an fp64 factor and extra rows, plain fp64 sums"""
        n, e = L.shape[0], E.shape[0]
        ld_, ss = float(np.sum(np.log(np.diag(L)))), float(np.sum(E * E))
        return ld_, ss, -0.5 * ss - e * ld_ - 0.5 * e * n * float(np.log(2 * np.pi))

    def lml_tol(self):
        """tolerance rule + the tree reduction's own rounding: depth 2^-53 sum |terms| (tests/test_gpu_ep.py)"""
        depth = 16 + (self.n + 255) // 256
        red = [depth * U * float(np.sum(np.abs(self.logdiag))), depth * U * float(self.sumsq)]
        red.append(0.5 * red[1] + self.e * red[0] + 4 * U * abs(float(self.lml_ref[2])))
        return [tol(e) + r for e, r in zip(self.e64["lml"], red)]


def lower_inverse_ld(L):
    """L^-1 in long double"""
    return xr.solve_lower(L, np.eye(L.shape[0], dtype=LD))


def cond2(A):
    s = np.linalg.eigvalsh(A)
    return float(s[-1] / s[0])


# ---------------------------------------------------------------------------------------------------------------------
# planted failures (exact `info`)
# ---------------------------------------------------------------------------------------------------------------------
INFO_N = 641
INFO_PIVOTS = (1, 16, 17, 128, 129, 256, 257, 384, 385, INFO_N)
INFO_NANS = ((20, 3), (300, 5), (300, 290))


def planted(n, pivots=(), nans=(), seed=0):
    """`well` (every pivot >= 0.5, so the expectation needs no reference) with P[j-1, j-1] = -1 for each 1-based j of `pivots` and
    A[i, c] = NaN (lower triangle, mirrored) for (i, c) of `nans` -> (matrix, expected info)."""
    P = well(n, seed)
    for j in pivots:
        P[j - 1, j - 1] = -1.0
    for i, c in nans:
        P[i, c] = P[c, i] = np.nan
    expect = min([j for j in pivots] + [i + 1 for i, _ in nans])
    return P, expect


def planted_cases():
    """(pivots, nans) for `planted` at n = INFO_N: one failure at every 16-, 128- and panel edge, two at once, NaN entries"""
    return [((j,), ()) for j in INFO_PIVOTS] + [((129, 400), ())] + [((), (ic,)) for ic in INFO_NANS]


def planted_ids():
    return ["pivot-" + "-".join(str(j) for j in p) if p else "nan-%d-%d" % n[0] for p, n in planted_cases()]
