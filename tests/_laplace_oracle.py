"""
TEST INFRASTRUCTURE ONLY (never imported by the package) -- a host statement of Laplace's approximation for GP
classification and counts (Rasmussen & Williams ch. 3 and 5.5) with a DENSE K, that shares nothing with the matrix-free
native path of gptorch_amd/models/laplace.py.  The reference has no such model (its Likelihood leaves the non-conjugate case
as a TODO), so nothing here restates reference code.

The algorithm is stated for two arithmetics:
  - dtype = np.float64: numpy with LAPACK's Cholesky and triangular solves, scipy.special's erfcx / log_ndtr / gammaln;
  - dtype = np.longdouble: tests/_xref's Cholesky, solves and direct-difference kernels; the probit terms, which numpy has
    no long-double functions for, come from mpmath at 30 digits and are rounded to long double.
Kernels take their distances by direct differences in both.

    psi(a) = sum lp(m + K a) - 1/2 a^T K a,   B = I + s K s (s = sqrt W),   b = W (f - m) + d1,   a+ = b - s B^-1 (s K b)
    a step is halved while psi_t < psi - 1e-10 (1 + |psi|), at most 10 times
    stop: max |delta f| <= tol (1 + max |f|)  (until_stall: go on until max |delta f| stops shrinking)
    log q = psi(a^) - sum log L_ii,  L the factor at the mode
    Sigma = K - K R K (R = s B^-1 s; the textbook dense form),  s2 = 1/2 diag(Sigma) d3,  u = s2 - R K s2
    G = 1/2 a a^T - 1/2 R + 1/2 (u d1^T + d1 u^T),  dlog q/dtheta = sum G dK/dtheta,  dlog q/dm = sum (d1 + u)
    predict_f: mean = m + K*^T a^,  cov = K** - V^T V,  V = L^-1 s K*
"""
import math

import numpy as np
import scipy.linalg
import scipy.special
import scipy.stats

from tests import _xref as xr

LD = xr.LD
PSI_SLACK = 1e-10
MAX_HALVINGS = 10
_S5, _S3 = math.sqrt(5.0), math.sqrt(3.0)


# ---- pointwise terms: (lp, d1, W, d3) per point ----------------------------------------------------------------------------------
def derivs64(lik, f, y):
    """the closed forms in plain fp64 (what the package's torch and HIP statements use)."""
    f, y = np.asarray(f, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if lik == "poisson":
        m = np.exp(f)
        return y * f - m - scipy.special.gammaln(y + 1.0), y - m, m, -m
    t = 2.0 * y - 1.0
    z = t * f
    if lik == "probit":
        zn, zp = np.minimum(z, 0.0), np.maximum(z, 0.0)
        neg = math.sqrt(2.0 / math.pi) / scipy.special.erfcx(-zn * math.sqrt(0.5))
        pos = np.exp(-0.5 * zp * zp) / math.sqrt(2.0 * math.pi) / (1.0 - 0.5 * scipy.special.erfc(zp * math.sqrt(0.5)))
        r = np.where(z < 0.0, neg, pos)
        zr = z + r
        return scipy.special.log_ndtr(z), t * r, r * zr, t * r * (zr * (zr + r) - 1.0)
    if lik == "logit":
        e = np.exp(-np.abs(f))
        q = 1.0 + e
        W = e / (q * q)
        return np.minimum(z, 0.0) - np.log1p(e), t * np.where(z >= 0.0, e, 1.0) / q, W, W * (np.sign(f) * -np.expm1(-np.abs(f)) / q)
    raise ValueError(lik)


def _mp_to_ld(v):
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


def derivs_mp(lik, f, y, dps=40):
    """the definitions themselves in mpmath (no tail tricks needed at `dps` digits) -> four lists of mpf."""
    import mpmath as mp
    out = ([], [], [], [])
    with mp.workdps(dps):
        for fi, yi in zip(np.asarray(f).ravel(), np.asarray(y).ravel()):
            fi = mp.mpf(float(fi)) + mp.mpf(float(LD(fi) - LD(float(fi))))
            yi = mp.mpf(float(yi))
            if lik == "poisson":
                m = mp.exp(fi)
                v = (yi * fi - m - mp.loggamma(yi + 1), yi - m, m, -m)
            else:
                t = 2 * yi - 1
                z = t * fi
                if lik == "probit":
                    Phi = mp.erfc(-z / mp.sqrt(2)) / 2
                    r = mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi) / Phi
                    v = (mp.log(Phi), t * r, r * (z + r), t * r * ((z + r) * (z + 2 * r) - 1))
                else:
                    sg = 1 / (1 + mp.exp(-fi))                      # sigma(f)
                    v = (-mp.log1p(mp.exp(-z)), t / (1 + mp.exp(z)), sg * (1 - sg), sg * (1 - sg) * (2 * sg - 1))
            for o, x in zip(out, v):
                o.append(x)
    return out


def derivs_ld(lik, f, y):
    f, y = np.asarray(f, dtype=LD), np.asarray(y, dtype=LD)
    if lik == "logit":
        t = 2 * y - 1
        z = t * f
        e = np.exp(-np.abs(f))
        q = 1 + e
        W = e / (q * q)
        return np.minimum(z, LD(0)) - np.log1p(e), t * np.where(z >= 0, e, LD(1)) / q, W, W * (np.sign(f) * -np.expm1(-np.abs(f)) / q)
    if lik == "poisson":
        m = np.exp(f)
        return y * f - m - _lgamma_ld(y), y - m, m, -m
    return tuple(np.array([_mp_to_ld(x) for x in col], dtype=LD) for col in derivs_mp(lik, f, y, dps=30))


_LGAMMA = {}


def _lgamma_ld(y):
    import mpmath as mp
    out = np.empty(y.shape, dtype=LD)
    for i, v in enumerate(y):
        k = float(v)
        if k not in _LGAMMA:
            with mp.workdps(30):
                _LGAMMA[k] = _mp_to_ld(mp.loggamma(mp.mpf(k) + 1))
        out[i] = _LGAMMA[k]
    return out


# ---- kernels by direct differences, either arithmetic -------------------------------------------------------------------------------
def kern(kind, X, X2, variance, ls, dt):
    """-> (K, B) with dK/dlog(ell_c) = B ((x_c - x2_c) / ell_c)^2; tests/_xref.k_of_r2 for long double, the same formulas in fp64."""
    if dt is LD:
        return xr.k_of_r2(kind, xr.scaled_sqdist(X, X2, ls), variance)
    X = np.asarray(X, dtype=np.float64)
    X2 = X if X2 is None else np.asarray(X2, dtype=np.float64)
    r2 = np.zeros((X.shape[0], X2.shape[0]))
    for c in range(X.shape[1]):
        t = (X[:, c:c + 1] - X2[None, :, c]) / ls[c]
        r2 += t * t
    v = float(variance)
    if kind == "Rbf":
        K = v * np.exp(-0.5 * r2)
        return K, K.copy()
    dead = r2 < xr.CLAMP
    r = np.sqrt(np.maximum(r2, xr.CLAMP))
    if kind == "Matern52":
        e = np.exp(-_S5 * r)
        K, B = v * (1.0 + _S5 * r + 5.0 / 3.0 * r * r) * e, v * (5.0 / 3.0) * (1.0 + _S5 * r) * e
    elif kind == "Matern32":
        e = np.exp(-_S3 * r)
        K, B = v * (1.0 + _S3 * r) * e, 3.0 * v * e
    elif kind in ("Exp", "Matern12"):
        K = v * np.exp(-r)
        B = K / r
    elif kind == "Periodic":
        K, B = v * np.cos(r), v * np.sin(r) / r
    else:
        raise ValueError(kind)
    return K, np.where(dead, 0.0, B)


class LaplaceOracle:
    """lik: "probit" | "logit" | "poisson"; kind: a stationary kind; variance, length_scales: CONSTRAINED values; mean: a float
    (Constant mean) or None.  Gradients are w.r.t. log variance, log length_scales [d or 1] and the mean."""

    def __init__(self, x, y, kind, lik, variance, length_scales, ARD=False, mean=None, dtype=np.float64):
        self.dt = LD if dtype is LD or dtype == np.longdouble else np.float64
        self.X = np.asarray(x, dtype=self.dt)
        self.y = np.asarray(y, dtype=self.dt).reshape(-1)
        self.n, self.d = self.X.shape
        self.kind, self.lik, self.ARD = kind, lik, ARD
        self.var = self.dt(variance)
        ls = np.atleast_1d(np.asarray(length_scales, dtype=self.dt))
        self.ls = ls if ls.size == self.d else np.full(self.d, ls[0], dtype=self.dt)
        self.m = self.dt(0.0 if mean is None else mean)
        self.Kf, self.Bf = kern(kind, self.X, None, self.var, self.ls, self.dt)
        self.a = None

    # -- arithmetic-specific pieces
    def derivs(self, f):
        return derivs_ld(self.lik, f, self.y) if self.dt is LD else derivs64(self.lik, f, self.y)

    def _chol(self, A):
        return xr.cholesky(A) if self.dt is LD else np.linalg.cholesky(A)

    def _lsolve(self, L, b):
        return xr.solve_lower(L, b) if self.dt is LD else scipy.linalg.solve_triangular(L, b, lower=True)

    def _ltsolve(self, L, b):
        return xr.solve_upper_t(L, b) if self.dt is LD else scipy.linalg.solve_triangular(L, b, lower=True, trans="T")

    def _factor(self, W):
        s = np.sqrt(np.maximum(W, self.dt(np.finfo(np.float64).tiny)))
        return s, self._chol(np.eye(self.n, dtype=self.dt) + s[:, None] * self.Kf * s[None, :])

    # -- the mode search
    def search(self, a0=None, tol=1e-8, max_iter=50, until_stall=False):
        dt, K = self.dt, self.Kf
        a = np.zeros(self.n, dtype=dt) if a0 is None else np.asarray(a0, dtype=dt).copy()
        Ka = K @ a
        f = self.m + Ka
        lp, d1, W, _ = self.derivs(f)
        psi = lp.sum() - dt(0.5) * (a @ Ka)
        steps = halvings = 0
        prev = None
        while True:
            if steps >= max_iter:
                raise RuntimeError("no convergence in %d steps" % max_iter)
            s, L = self._factor(W)
            b = W * Ka + d1
            a_new = b - s * self._ltsolve(L, self._lsolve(L, s * (K @ b)))
            Ka_new = K @ a_new
            t = dt(1.0)
            for h in range(MAX_HALVINGS + 1):
                a_t = a_new if t == 1 else a + t * (a_new - a)
                Ka_t = Ka_new if t == 1 else Ka + t * (Ka_new - Ka)
                f_t = self.m + Ka_t
                with np.errstate(over="ignore", invalid="ignore"):
                    lp_t, d1_t, W_t, _ = self.derivs(f_t)
                    psi_t = lp_t.sum() - dt(0.5) * (a_t @ Ka_t)
                if psi_t >= psi - dt(PSI_SLACK) * (1 + abs(psi)) or h == MAX_HALVINGS:
                    break
                t = t / 2
                halvings += 1
            max_df, max_f = np.max(np.abs(f_t - f)), np.max(np.abs(f_t))
            a, Ka, f, d1, W, psi = a_t, Ka_t, f_t, d1_t, W_t, psi_t
            steps += 1
            if until_stall:
                if max_df == 0 or (prev is not None and max_df <= tol * (1 + max_f) and max_df >= prev):
                    break
                prev = max_df
            elif max_df <= tol * (1 + max_f):
                break
        self.a, self.Ka, self.f, self.steps, self.halvings = a, Ka, f, steps, halvings
        self.lp, self.d1, self.W, self.d3 = self.derivs(f)
        self.s, self.L = self._factor(self.W)
        return self

    def log_evidence(self):
        return self.lp.sum() - self.dt(0.5) * (self.a @ self.Ka) - np.sum(np.log(np.diag(self.L)))

    def loss(self):
        return -self.log_evidence()

    def loss_grads(self):
        """-> [d loss/d log variance [1], d loss/d log length_scales [d or 1], d loss/d mean [1]] at the mode found."""
        dt, K, s = self.dt, self.Kf, self.s
        Li = self._lsolve(self.L, np.eye(self.n, dtype=dt))
        R = s[:, None] * (Li.T @ Li) * s[None, :]
        KR = K @ R
        sigma = np.diag(K) - np.einsum("ij,ji->i", KR, K)
        s2 = dt(0.5) * sigma * self.d3
        u = s2 - R @ (K @ s2)
        G = dt(0.5) * (np.outer(self.a, self.a) - R + np.outer(u, self.d1) + np.outer(self.d1, u))
        g_ls = np.empty(self.d, dtype=dt)
        GB = G * self.Bf
        for c in range(self.d):
            t = (self.X[:, c:c + 1] - self.X[None, :, c]) / self.ls[c]
            g_ls[c] = np.sum(GB * t * t)
        g_var = np.array([np.sum(G * K)])
        return [-g_var, -(g_ls if self.ARD else np.array([g_ls.sum()])), -np.array([np.sum(self.d1 + u)])]

    def predict_f(self, x_new, diag=True):
        Ks = kern(self.kind, self.X, np.asarray(x_new, dtype=self.dt), self.var, self.ls, self.dt)[0]
        mean = self.m + Ks.T @ self.a
        V = self._lsolve(self.L, self.s[:, None] * Ks)
        if diag:
            return mean, self.var - np.sum(V * V, 0)
        return mean, kern(self.kind, np.asarray(x_new, dtype=self.dt), None, self.var, self.ls, self.dt)[0] - V.T @ V


# ---- the golden cases (tests/golden/make_laplace_golden.py writes them, the tests rebuild inputs and models from them) ----------
def case_inputs(case):
    """x [n, d], y [n, 1], xs [40, d] of a case from gptorch_amd.rng: x ~ N(0, 1), a smooth latent g(x), labels / counts drawn
    with the generator's uniforms."""
    from gptorch_amd import rng
    n, d, seed = int(case["n"]), int(case["d"]), int(case["seed"])
    x = rng.normal(seed, (n, d))
    g = np.sin(1.3 * x[:, 0]) + 0.7 * np.cos(x[:, 1:].sum(1)) + 0.3 * x[:, 0]
    u = rng.uniform(seed + 1, n)
    if case["lik"] == "poisson":
        y = scipy.stats.poisson.ppf(u, np.exp(float(case["offset"]) + float(case["gain"]) * g))
    else:
        p = scipy.special.ndtr(1.5 * g) if case["lik"] == "probit" else scipy.special.expit(2.5 * g)
        y = (u < p).astype(np.float64)
    return {"x": x, "y": y.reshape(n, 1), "xs": rng.normal(seed + 2, (40, d))}


def build_oracle(case, inp, dtype=np.float64):
    return LaplaceOracle(inp["x"], inp["y"], case["kind"], case["lik"], case["variance"], case["length_scales"], ARD=bool(case["ARD"]),
                         mean=case["mean"], dtype=dtype)


def build_model(case, inp):
    import torch
    from gptorch_amd import kernels, likelihoods, mean_functions
    from gptorch_amd.models import LaplaceGP
    d = int(case["d"])
    ls = np.asarray(case["length_scales"], dtype=np.float64) if case["ARD"] else float(np.atleast_1d(case["length_scales"])[0])
    k = getattr(kernels, case["kind"])(d, variance=float(case["variance"]), length_scales=ls, ARD=bool(case["ARD"]))
    lik = likelihoods.Poisson() if case["lik"] == "poisson" else likelihoods.Bernoulli(case["lik"])
    mean = None if case["mean"] is None else mean_functions.Constant(1, torch.tensor([float(case["mean"])], dtype=torch.float64))
    return LaplaceGP(inp["x"], inp["y"], k, lik, mean_function=mean)
