"""
TEST INFRASTRUCTURE ONLY -- which kernel kinds every kind-dispatched entry point of include/gpnative.h serves, one small input
set for all of them, and the reference of each entry's output for a NAMED kind, stated once for two arithmetics (numpy long
double and plain fp64).  Host only: nothing here touches the GPU.

The long-double kernels are tests/_xref.k_of_r2 on tests/_xref.scaled_sqdist (through tests/_laplace_oracle.kern, which holds
the same closed forms in fp64); SqDist is K = r^2 with B = -(dK/dr) / r = -2 and no variance.  The fp64 statement of the same
sums gives e64, the error a plain fp64 evaluation makes, and xr.tol(e64, what) the tolerance -- nothing comes from the code
under test.  tests/test_kind_ref_host.py checks that the six kinds' references lie at least SEPARATION tolerances apart for
every output, so a call that ran another kind's instantiation cannot pass.

gptorch_amd never imports this module.
"""
import numpy as np

from gptorch_amd import rng
from tests import _laplace_oracle as lo
from tests import _refine_ref as rr
from tests import _xref as xr

LD = xr.LD
KIND_NAMES = {0: "Rbf", 1: "Matern52", 2: "Matern32", 3: "Exp", 4: "SqDist", 5: "Periodic"}
KIND_IDS = tuple(KIND_NAMES)
BAD_KINDS = (-1, 6)
COVARIANCES = (0, 1, 2, 3, 5)              # the kinds that are covariance functions
WITH_SQDIST = (0, 1, 2, 3, 4, 5)
SEPARATION = 1e6

# entry point -> the kinds it serves; every other value of `kind` is refused with a negative status before any launch
# (mirrored in each entry's comment in include/gpnative.h)
SERVED = {}
for _name in ("gpn_kernel_matrix", "gpn_kernel_matrix_batched", "gpn_kernel_grad", "gpn_kernel_grad_batched", "gpn_kernel_grad_x2",
              "gpn_kernel_grad_x2_batched", "gpn_lml_grad", "gpn_lml_grad_batched", "gpn_loo_grad", "gpn_loo_grad_batched"):
    SERVED[_name] = WITH_SQDIST
for _name in ("gpn_lml_forward", "gpn_lml_forward_saving", "gpn_lml_forward_batched", "gpn_lml_forward_ragged", "gpn_lml_backward",
              "gpn_lml_backward_batched", "gpn_lml_backward_ragged", "gpn_lml_refine", "gpn_refine_resid_part", "gpn_predict",
              "gpn_predict_blocked", "gpn_laplace_system", "gpn_laplace_matvec", "gpn_laplace_diag", "gpn_laplace_grad",
              "gpn_laplace_system_batched", "gpn_laplace_matvec_batched", "gpn_laplace_diag_batched", "gpn_laplace_grad_batched",
              "gpn_dist_lml_forward", "gpn_dist_lml_grad", "gpn_dist_lml_refine", "gpn_dist_predict"):
    SERVED[_name] = COVARIANCES

# ---- the one shape ------------------------------------------------------------------------------------------------------------------
N, M, D, DY, BATCH = 65, 63, 2, 2, 3        # two 64-row tiles, an X2 of another length, ARD, two right-hand sides, three models


class Inputs:
    """everything the dispatch matrix feeds the entry points, as fp64 numpy arrays.  Points: tests/_refine_ref.points (repeated
    rows, pairs under and just above the clamp, a row 1000 ell away, rows at pi/2 +- 1e-3 and pi +- 1e-3); the rest from
    gptorch_amd.rng.  Model b of the lock-step forms has its own variance[b], length_scales[b] (ARD) and noise[b]; the noise is
    large enough that K + noise I is positive definite for the indefinite Periodic kernel as well (the host test factors it)."""

    def __init__(self):
        self.n, self.m, self.d, self.dy, self.batch = N, M, D, DY, BATCH
        self.ls = np.stack([rr.length_scales(D, True, 11 + b, 1.0 + 0.05 * b) for b in range(BATCH)])           # [batch, d]
        self.var = np.array([1.3 * (1.0 + 0.1 * b) for b in range(BATCH)])
        self.noise = np.array([40.0 + b for b in range(BATCH)])          # lambda_min(K_Periodic) = -22.3, -12.6, -19.4 here
        self.X = rr.points(21, N, D, self.ls[0, 0])
        self.X2 = rr.points(22, M, D, self.ls[0, 0], first=1)
        # smooth targets of some size: the quadratic form then leans on K's leading eigenvectors, where the kinds differ most
        xc = np.clip(self.X, -3.0, 3.0)
        self.Y = 10.0 * np.sin(xc[:, :1] + np.arange(DY)[None, :]) + 5.0 * np.cos(xc[:, 1:2]) + rng.normal(23, (N, DY))
        self.G = rng.normal(24, (BATCH, N, M))                           # dense weights of gpn_kernel_grad / _x2
        self.scale = 0.75                                                # gpn_kernel_grad_x2's scale
        self.P = np.stack([spd(N, 30 + b) for b in range(BATCH)])        # stands for Kyy^-1 / Q / B^-1 (lower triangle read)
        self.at = rng.normal(40, (BATCH, DY, N))                         # a^T
        self.wt = rng.normal(41, (BATCH, DY, N))                         # w^T
        self.s = 0.05 + 2.0 * rng.uniform(42, BATCH * N).reshape(BATCH, N)   # sqrt W
        self.vec = rng.normal(43, (BATCH, 4, N))                         # v / a, u, d1 of the Laplace entries

    def hyp(self, b):
        return self.var[b], self.ls[b], self.noise[b]


def spd(n, seed):
    g = rng.normal(seed, (n, n + 3))
    return g @ g.T / (n + 3) + 0.5 * np.eye(n)


_INPUTS = None


def inputs():
    global _INPUTS
    if _INPUTS is None:
        _INPUTS = Inputs()
    return _INPUTS


# ---- kernels and sweeps, either arithmetic ----------------------------------------------------------------------------------------
def sqdist(X, X2, ls, dt):
    if dt is LD:
        return xr.scaled_sqdist(X, X2, ls)
    X = np.asarray(X, dtype=np.float64)
    X2 = X if X2 is None else np.asarray(X2, dtype=np.float64)
    r2 = np.zeros((X.shape[0], X2.shape[0]))
    for c in range(X.shape[1]):
        t = (X[:, c:c + 1] - X2[None, :, c]) / ls[c]
        r2 += t * t
    return r2


def kern(kind, X, X2, var, ls, dt):
    """(K, B) of a named kind with dK/dlog(ell_c) = B ((x_c - x2_c) / ell_c)^2 and dK/dx2_c = B (x_c - x2_c) / ell_c^2."""
    if kind == "SqDist":
        r2 = sqdist(X, X2, ls, dt)
        return r2, np.full(r2.shape, dt(-2))
    return lo.kern(kind, X, X2, var, np.asarray(ls, dtype=dt), dt)


def param_grads(kind, X, X2, var, ls, W, dt):
    """sum W dK/d(variance, length_scales [d]) w.r.t. the CONSTRAINED values."""
    Km, B = kern(kind, X, X2, var, ls, dt)
    W = np.asarray(W, dtype=dt)
    X = np.asarray(X, dtype=dt)
    X2 = X if X2 is None else np.asarray(X2, dtype=dt)
    out = np.empty(1 + X.shape[1], dtype=dt)
    out[0] = 0 if kind == "SqDist" else np.sum(W * Km) / dt(var)
    WB = W * B
    for c in range(X.shape[1]):
        t = (X[:, c:c + 1] - X2[None, :, c]) / dt(ls[c])
        out[1 + c] = np.sum(WB * t * t) / dt(ls[c])
    return out


def x2_grads(kind, X, X2, var, ls, W, scale, dt):
    """scale * sum_i W_ij dK(x_i, z_j)/dz_jc [m, d]."""
    B = kern(kind, X, X2, var, ls, dt)[1]
    WB = np.asarray(W, dtype=dt) * B
    X, X2 = np.asarray(X, dtype=dt), np.asarray(X2, dtype=dt)
    out = np.empty(X2.shape, dtype=dt)
    for c in range(X.shape[1]):
        t = (X[:, c:c + 1] - X2[None, :, c]) / (dt(ls[c]) * dt(ls[c]))
        out[:, c] = dt(scale) * np.sum(WB * t, axis=0)
    return out


def _chol(A, dt):
    return xr.cholesky(A) if dt is LD else np.linalg.cholesky(A)


def _lsolve(L, b, dt):
    import scipy.linalg
    return xr.solve_lower(L, b) if dt is LD else scipy.linalg.solve_triangular(L, b, lower=True)


def _ltsolve(L, b, dt):
    import scipy.linalg
    return xr.solve_upper_t(L, b) if dt is LD else scipy.linalg.solve_triangular(L, b, lower=True, trans="T")


# ---- the reference of every output, by family of entry points ------------------------------------------------------------------------
# Each returns {output name: (array, what, metric)}: `what` keys xr.tol, metric "abs" (xr.abs_err) or "rel" (xr.rel_err).
def ref_kernel_matrix(kind, b, dt, inp=None):
    inp = inp or inputs()
    var, ls, _ = inp.hyp(b)
    # r^2 reaches 1e6 on the planted far row: SqDist entries are judged relative to the largest, the covariances absolutely
    return {"K": (kern(kind, inp.X, inp.X2, var, ls, dt)[0], "K", "rel" if kind == "SqDist" else "abs")}


def ref_kernel_grad(kind, b, dt, inp=None):
    inp = inp or inputs()
    var, ls, _ = inp.hyp(b)
    return {"out": (param_grads(kind, inp.X, inp.X2, var, ls, inp.G[b], dt), "dense_grad", "rel")}


def ref_kernel_grad_x2(kind, b, dt, inp=None):
    inp = inp or inputs()
    var, ls, _ = inp.hyp(b)
    return {"out": (x2_grads(kind, inp.X, inp.X2, var, ls, inp.G[b], inp.scale, dt), "point_grad", "rel")}


def _sweep_with_trace(kind, b, Gm, dt, inp):
    var, ls, _ = inp.hyp(b)
    return np.concatenate([param_grads(kind, inp.X, None, var, ls, Gm, dt), [np.trace(Gm)]])


def ref_lml_grad(kind, b, dt, inp=None):
    """G = 1/2 (a a^T - dy Kinv) from the given Kinv (inp.P) and a^T (inp.at)."""
    inp = inp or inputs()
    a = inp.at[b].astype(dt).T
    Gm = dt(0.5) * (a @ a.T - inp.dy * inp.P[b].astype(dt))
    return {"out": (_sweep_with_trace(kind, b, Gm, dt, inp), "dense_grad", "rel")}


def ref_loo_grad(kind, b, dt, inp=None):
    """G = -Q + 1/2 (a w^T + w a^T) from the given Q (inp.P), a^T and w^T."""
    inp = inp or inputs()
    a, w = inp.at[b].astype(dt).T, inp.wt[b].astype(dt).T
    Gm = -inp.P[b].astype(dt) + dt(0.5) * (a @ w.T + w @ a.T)
    return {"out": (_sweep_with_trace(kind, b, Gm, dt, inp), "dense_grad", "rel")}


class GP:
    """GPR.log_likelihood, its closed-form backward and predict for model b in arithmetic dt (zero mean)."""

    def __init__(self, kind, b, dt, inp=None):
        inp = inp or inputs()
        self.inp, self.kind, self.b, self.dt = inp, kind, b, dt
        var, ls, noise = inp.hyp(b)
        self.Kyy = kern(kind, inp.X, None, var, ls, dt)[0] + dt(noise) * np.eye(inp.n, dtype=dt)
        self.L = _chol(self.Kyy, dt)
        self.alpha = _lsolve(self.L, inp.Y.astype(dt), dt)

    def out3(self):
        dt, inp = self.dt, self.inp
        logdet, quad = np.sum(np.log(np.diag(self.L))), np.sum(self.alpha ** 2)
        return np.array([logdet, quad, -dt(0.5) * quad - inp.dy * logdet - dt(0.5) * inp.dy * inp.n * np.log(2 * dt(np.pi))], dtype=dt)

    def backward(self):
        dt, inp = self.dt, self.inp
        a = _ltsolve(self.L, self.alpha, dt)
        Li = _lsolve(self.L, np.eye(inp.n, dtype=dt), dt)
        Gm = dt(0.5) * (a @ a.T - inp.dy * (Li.T @ Li))
        return _sweep_with_trace(self.kind, self.b, Gm, dt, inp), -a

    def predict(self):
        dt, inp = self.dt, self.inp
        var, ls, _ = inp.hyp(self.b)
        A = _lsolve(self.L, kern(self.kind, inp.X, inp.X2, var, ls, dt)[0], dt)
        mean = A.T @ self.alpha
        return mean, dt(var) - np.sum(A * A, 0), kern(self.kind, inp.X2, None, var, ls, dt)[0] - A.T @ A


def ref_lml(kind, b, dt, inp=None):
    """out3, grads, grad_resid, mean, var, cov of the whole-path entries, and Kyy a_given of gpn_refine_resid_part."""
    inp = inp or inputs()
    gp = GP(kind, b, dt, inp)
    grads, resid = gp.backward()
    mean, var, cov = gp.predict()
    return {"out3": (gp.out3(), "loss", "rel"), "grads": (grads, "grad", "rel"), "grad_resid": (resid, "grad", "rel"),
            "mean": (mean, "mean", "abs"), "var": (var, "var", "abs"), "cov": (cov, "var", "abs"),
            "ka": (inp.at[b].astype(dt) @ gp.Kyy, "dense_grad", "rel")}


def ref_laplace(kind, b, dt, inp=None):
    inp = inp or inputs()
    var, ls, _ = inp.hyp(b)
    K = kern(kind, inp.X, None, var, ls, dt)[0]
    s, Binv = inp.s[b].astype(dt), inp.P[b].astype(dt)
    v, a, u, d1 = (inp.vec[b, k].astype(dt) for k in range(4))
    Gm = dt(0.5) * (np.outer(a, a) - s[:, None] * Binv * s[None, :] + np.outer(u, d1) + np.outer(d1, u))
    return {"system": (np.eye(inp.n, dtype=dt) + s[:, None] * K * s[None, :], "K", "rel"),
            "matvec": (K @ v, "dense_grad", "rel"),
            "diag": (np.sum(K * Binv * s[None, :], 1) / s, "dense_grad", "rel"),
            "grad": (param_grads(kind, inp.X, None, var, ls, Gm, dt), "dense_grad", "rel")}


FAMILIES = {"kernel_matrix": (ref_kernel_matrix, WITH_SQDIST), "kernel_grad": (ref_kernel_grad, WITH_SQDIST),
            "kernel_grad_x2": (ref_kernel_grad_x2, WITH_SQDIST), "lml_grad": (ref_lml_grad, WITH_SQDIST),
            "loo_grad": (ref_loo_grad, WITH_SQDIST), "lml": (ref_lml, COVARIANCES), "laplace": (ref_laplace, COVARIANCES)}


def metric(got, want, how):
    return xr.abs_err(got, want) if how == "abs" else xr.rel_err(got, want)


_REFS = {}


def reference(family, kind_id, b):
    """{output: (long-double value, tolerance, metric)} of model b for the kind with this id; computed once."""
    key = (family, kind_id, b)
    if key not in _REFS:
        fn = FAMILIES[family][0]
        kind = KIND_NAMES[kind_id]
        hi, lo64 = fn(kind, b, LD), fn(kind, b, np.float64)
        _REFS[key] = {name: (val, xr.tol(metric(lo64[name][0], val, how), what), how) for name, (val, what, how) in hi.items()}
    return _REFS[key]


# ---- the ragged LML forms: more than 256 rows, models of different lengths ---------------------------------------------------------------
RAGGED_N, RAGGED_N_OF, RAGGED_D = 289, (289, 257), 1      # two models; d = 1, where Periodic is positive semi-definite: a small noise
                                                         # keeps the kinds far apart at this size


class RaggedModel:
    """model b of the ragged batch as an Inputs-like object for GP: the first RAGGED_N_OF[b] of the shared planted points."""

    def __init__(self, b):
        full = ragged_inputs()
        self.n, self.d, self.dy = RAGGED_N_OF[b], RAGGED_D, DY
        self.X, self.Y = full["X"][:self.n], full["Y"][:self.n]
        self.X2 = self.X[:8]                                     # (GP.predict's test points: unused here)
        self._hyp = (full["var"][b], full["ls"][b], full["noise"][b])

    def hyp(self, b):
        return self._hyp


_RAGGED = None


def ragged_inputs():
    global _RAGGED
    if _RAGGED is None:
        B = len(RAGGED_N_OF)
        ls = np.array([[0.9 + 0.2 * b] for b in range(B)])
        X = rr.points(51, RAGGED_N, RAGGED_D, ls[0, 0])
        xc = np.clip(X, -3.0, 3.0)
        Y = 3.0 * np.sin(xc[:, :1] + np.arange(DY)[None, :]) + rng.normal(52, (RAGGED_N, DY))
        _RAGGED = {"X": X, "Y": Y, "ls": ls, "var": np.array([1.3 * (1.0 + 0.1 * b) for b in range(B)]),
                   "noise": np.array([0.5 + 0.1 * b for b in range(B)])}
    return _RAGGED


def ref_ragged(kind, b, dt, inp=None):
    gp = GP(kind, b, dt, RaggedModel(b))
    return {"out3": (gp.out3(), "loss", "rel"), "grads": (gp.backward()[0], "grad", "rel")}


FAMILIES["ragged"] = (ref_ragged, COVARIANCES)
RAGGED_BATCH = len(RAGGED_N_OF)
