"""
TEST INFRASTRUCTURE ONLY -- long-double statements of the two sparse bounds and of the FITC likelihood, their gradients
and predictions.

    VFERef    the collapsed bound of sparse_gpr.py:108-153 (Titsias), predict_f of 155-195
    SVGPRef   q(f)'s marginals, KL(q(u) || p(u)), the minibatch-scaled Gaussian data term and the bound of
              sparse_gpr.py:198-381
    FITCRef   the marginal likelihood of gptorch_amd/models/_fitc.py's header in its whitened form (A = L^-1 Kuf,
              lambda = Kdiag - colsum(A^2) + s, B = I + A D A^T, c = LB^-1 A D err) and the collapsed predictions; its
              gradients by matrix calculus on (A, lambda, err), NOT the collapsed S of _fitc.py

Everything is numpy long double on top of tests/_xref.py (direct-difference distances with the reference's clamp, its
Cholesky and triangular solves, its closed-form kernel pull-backs).  Nothing here is shared with gptorch_amd.  The
gradients differentiate the bounds as functions of the whitened quantities (A = L^-1 Kuf, ...) by matrix calculus and
pull each triangular solve back onto Kuf and, through the Cholesky factor, onto Kuu WITHOUT the symmetry shortcuts and
the collapsed M x M expressions of gptorch_amd/models/sparse_gpr.py (the N-sized product G_A A^T is formed as it
stands); dF/dKuu, dF/dKuf, dF/dKdiag then go through _xref's kernel-gradient functions.  tests/test_sparse_ref_host.py
checks every gradient by long-double central differences and by fp64 autograd before any GPU test relies on it.

Parameters are the constrained values; gradients are of the LOSS (minus the bound) w.r.t. the raw values the optimisers
see: the log of every positive value, the mean and Z as they are, and for q_sqrt the strictly-lower entries as they
are with the log of the diagonal.

Direct64VFE / Direct64SVGP / Direct64FITC are the plain fp64 evaluations (the reference's op chain in torch on the CPU
-- FITC: the M-sized Woodbury form of tests/_fitc_oracle.py --, K by direct differences, gradients by autograd) whose
distance from the long-double value is the e64 of tests/_xref.tol.

`plant=` evaluates a reference WITH one deliberate mistake, for the resolving-power tests only:
    VFE   "drop_last_row"     the last row of x is missing from A A^T and A err (N, |err|^2 and tr Kff still count it)
          "drop_k_slice"      16 columns of A (rows plant_at .. plant_at + 15 of x) are missing from A A^T alone
          "trkff_one_chunk"   tr Kff over the first plant_at rows only
          "gq_triangle"       the symmetric M x M matrix that multiplies Kuf in dF/dKuf held as its lower triangle only
    SVGP  "scale_one"         the minibatch scale num_data / rows replaced by 1
          "gq_triangle"       G_Q = alpha^T diag(g_var) alpha held as its lower triangle only (not mirrored)
          "drop_kd_diag"      the -dy / diag(S_L) term of d KL / d S_L dropped
    FITC  "drop_last_row"     the last row of x is missing from A D A^T and A D err (sum log lambda, sum err^2 / lambda still count it)
          "sums_first_chunk"  sum log lambda_i and sum err_i^2 / lambda_i over the first plant_at rows only (one chunk's slot lost)
          "aga_triangle"      the A diag(g) A^T part of T = G_A A^T held as its lower triangle only, where Psi mirrors it
          "drop_kdiag_grad"   the dF/dKdiag pull-back dropped
          "g_without_h"       g_i without its a_i^T B^-1 a_i / lambda_i^2 term
"""
import math

import numpy as np
import torch

from oracle import gp_oracle as orc
from tests import _fitc_oracle as fo
from tests import _svgp_oracle as so
from tests import _xref as xr

LD = xr.LD
COMPOSITE = "Linear+Rbf+Constant"
LOG2PI = np.log(2 * LD(np.pi))


# ---------------------------------------------------------------------------------------------------------------------
# kernels: the dict form of tests/_svgp_oracle.py -> an _xref spec, and the pull-backs _xref does not have
# ---------------------------------------------------------------------------------------------------------------------
def spec_of(kernel, d):
    """dict(kind=<stationary kind>, variance, length_scales [, ARD]) or dict(kind="Linear+Rbf+Constant", linear_variance,
    variance, length_scales, constant) -> spec; leaf ids are the gradient names of the stationary / Rbf leaf's owner."""
    if kernel["kind"] == COMPOSITE:
        return [[xr.leaf("linear_variance", "linear", variance=xr.ld(kernel["linear_variance"]) * np.ones(d), ard=True)],
                [xr.leaf("k", "stationary", "Rbf", kernel["variance"], np.atleast_1d(kernel["length_scales"]), False)],
                [xr.leaf("constant", "constant", variance=kernel["constant"])]]
    ard = bool(kernel.get("ARD"))
    ls = xr.ld(kernel["length_scales"]) * (np.ones(d) if ard else np.ones(1))       # (long double kept: central differences)
    return [[xr.leaf("k", "stationary", kernel["kind"], kernel["variance"], ls, ard)]]


def kdiag_param_grads(spec, X, w):
    """d sum(w * Kdiag(X)) / d log variance(s) -> {id: g_var} (no leaf's diagonal depends on a length scale)."""
    X, w = xr.ld(X), xr.ld(w)
    out = {}
    for g in spec:
        diags = [xr.leaf_Kdiag(l, X) for l in g]
        for ti, l in enumerate(g):
            wt = w.copy()
            for ui, dg in enumerate(diags):
                if ui != ti:
                    wt = wt * dg
            if l["type"] == "linear":
                v = xr._lin_v(l, X.shape[1])
                gv = np.array([v[c] * np.sum(wt * X[:, c] * X[:, c]) for c in range(X.shape[1])], dtype=LD)
                gv = gv if np.size(l["variance"]) > 1 or l["ard"] else np.array([gv.sum()])
            else:
                gv = np.array([LD(l["variance"]) * np.sum(wt)])
            out[l["id"]] = out[l["id"]] + gv if l["id"] in out else gv
    return out


def point_grads(spec, Xa, Xb, W):
    """d sum(W * K(Xa, Xb)) / dXa (Xb None: K(Xa), through both arguments) for a SUM of single leaves."""
    Xa, W = xr.ld(Xa), xr.ld(W)
    g = np.zeros(Xa.shape, dtype=LD)
    for grp in spec:
        if len(grp) != 1:
            raise ValueError("point gradients: sums of single leaves only")
        l = grp[0]
        if l["type"] == "stationary":
            r = xr.kernel_point_grads(l["kind"], Xa, Xb, l["variance"], l["length_scales"], W)
            g += r if Xb is None else r[0]
        elif l["type"] == "linear":
            v = xr._lin_v(l, Xa.shape[1])
            g += ((W + W.T) @ Xa if Xb is None else W @ xr.ld(Xb)) * v
    return g


def _kernel_grads(spec, terms, kdiag_terms):
    """sum of the pull-backs of [(Xa, Xb, W)] and [(X, w)] onto every leaf's raw parameters -> {name: gradient}."""
    acc = {}
    for Xa, Xb, W in terms:
        for i, (gv, gl) in xr.expr_param_grads(spec, Xa, Xb, W).items():
            acc[i] = (acc[i][0] + gv, acc[i][1] + gl) if i in acc else (gv, gl)
    for X, w in kdiag_terms:
        for i, gv in kdiag_param_grads(spec, X, w).items():
            acc[i] = (acc[i][0] + gv, acc[i][1])
    out = {}
    for i, (gv, gl) in acc.items():
        if i == "k":
            out["variance"], out["length_scales"] = gv, gl
        else:
            out[i] = gv
    return out


def _inverse_from_factor(L):
    """(L^-1, (L L^T)^-1)."""
    Li = xr.solve_lower(L, np.eye(L.shape[0], dtype=LD))
    return Li, Li.T @ Li


# ---------------------------------------------------------------------------------------------------------------------
# VFE
# ---------------------------------------------------------------------------------------------------------------------
class VFERef:
    def __init__(self, x, y, z, kernel, noise, mean=None, jitter=0.0, plant=None, plant_at=0):
        self.X, self.Y, self.Z = xr.ld(x), xr.ld(y), xr.ld(z)
        self.n, self.p = self.Y.shape
        self.m = self.Z.shape[0]
        self.spec = spec_of(kernel, self.X.shape[1]) if isinstance(kernel, dict) else kernel
        self.s = LD(noise)
        self.mean = np.zeros(self.p, dtype=LD) if mean is None else xr.ld(mean)
        self.err = self.Y - self.mean
        self.plant = plant
        # column masks of Kuf: what enters C = Kuf Kfu (A A^T) and what enters v = Kuf err (A err)
        self.mask_c, self.mask_v = np.ones(self.n, dtype=LD), np.ones(self.n, dtype=LD)
        self.mask_d = np.ones(self.n, dtype=LD)                    # rows counted in tr Kff
        if plant == "drop_last_row":
            self.mask_c[-1] = self.mask_v[-1] = 0
        elif plant == "drop_k_slice":
            self.mask_c[plant_at:plant_at + 16] = 0
        elif plant == "trkff_one_chunk":
            self.mask_d[plant_at:] = 0
        elif plant not in (None, "gq_triangle"):
            raise ValueError(plant)
        self.Kuu = xr.expr_K(self.spec, self.Z, None) + LD(jitter) * np.eye(self.m, dtype=LD)
        self.Kuf = xr.expr_K(self.spec, self.Z, self.X)
        self.trkff = np.sum(xr.expr_Kdiag(self.spec, self.X) * self.mask_d)
        self.L = xr.cholesky(self.Kuu)
        A = xr.solve_lower(self.L, self.Kuf)
        self.Ac = A * self.mask_c
        self.AAT = self.Ac @ self.Ac.T / self.s
        self.Aerr = (A * self.mask_v) @ self.err
        self.LB = xr.cholesky(self.AAT + np.eye(self.m, dtype=LD))
        self.c = xr.solve_lower(self.LB, self.Aerr) / self.s

    def bound(self):
        """sparse_gpr.py:139-151."""
        n, p, s = self.n, self.p, self.s
        return (-LD(0.5) * p * n * LOG2PI - p * np.sum(np.log(np.diag(self.LB))) - LD(0.5) * p * n * np.log(s)
                - LD(0.5) * (np.sum(self.err ** 2) + p * self.trkff) / s + LD(0.5) * np.sum(self.c ** 2)
                + LD(0.5) * p * np.trace(self.AAT))

    def loss(self):
        return -self.bound()

    def loss_grads(self, with_Z=True):
        """-> {variance, length_scales (composite: + linear_variance, constant), noise, mean, Z}: d loss / d raw.

        The bound as a function of the whitened A = L^-1 Kuf (A_c: the columns that enter A A^T, A_v: those that enter v = A err),
        B = I + A_c A_c^T / s, b = B^-1 v / s:
            dF/dA_c = [p (I - B^-1) - b b^T] A_c / s,   dF/dA_v = b err^T / s,   G_A = their sum
            dF/ds   = p/(2s) tr(I - B^-1) - |c|^2/s + b^T (B - I) b/(2s) - p tr(A_c A_c^T)/(2 s^2) - pN/(2s) + (|err|^2 + p tr Kff)/(2 s^2)
            dF/derr = -(err - A_v^T b)/s,   dF/dmean = -sum over rows of it,   dF/dKdiag = -p/(2s)
        and A = L^-1 Kuf pulled back: dKuf = L^-T G_A, and onto L through dA = -Phi(W) A, W = L^-1 dKuu L^-T, Phi = lower triangle
        with half the diagonal: with T = G_A A^T (NOT assumed symmetric) dF = -sum(T * Phi(W)) = -tr(Psi(T) W),
        Psi(T) = 1/2 (strict lower + its mirror + diagonal), so dKuu = -L^-T Psi(T) L^-1.  (A first version of this method worked
        over Kuu^-1 and D = s Kuu + Kuf Kfu instead: right, but dF/dKuu there is a difference of terms cond(Kuu) times its size, and
        the gradients came out with ~1e-10 of noise -- more than the native path's own error.)"""
        n, p, m, s = self.n, self.p, self.m, self.s
        eye = np.eye(m, dtype=LD)
        Li = xr.solve_lower(self.L, eye)
        Binv = _inverse_from_factor(self.LB)[1]
        A = xr.solve_lower(self.L, self.Kuf)
        Av = A * self.mask_v
        b = Binv @ self.Aerr / s
        GQ = p * (eye - Binv) - b @ b.T
        if self.plant == "gq_triangle":
            GQ = np.tril(GQ)
        GA = (GQ @ self.Ac) * self.mask_c / s + (b @ self.err.T / s) * self.mask_v
        T = GA @ A.T
        Psi = LD(0.5) * (np.tril(T, -1) + np.tril(T, -1).T + np.diag(np.diag(T)))
        Guu = -Li.T @ Psi @ Li
        Guf = Li.T @ GA
        g_s = (LD(0.5) * p / s * (m - np.trace(Binv)) - np.sum(self.c ** 2) / s + LD(0.5) * np.sum(b * ((self.AAT) @ b)) / s
               - LD(0.5) * p * np.trace(self.AAT) / s - LD(0.5) * p * n / s + LD(0.5) * (np.sum(self.err ** 2) + p * self.trkff) / (s * s))
        g_err = -(self.err - Av.T @ b) / s
        out = _kernel_grads(self.spec, [(self.Z, None, Guu), (self.Z, self.X, Guf)], [(self.X, -LD(0.5) * p / s * self.mask_d)])
        out["noise"] = np.array([s * g_s])
        out["mean"] = -g_err.sum(0)
        if with_Z:
            out["Z"] = point_grads(self.spec, self.Z, None, Guu) + point_grads(self.spec, self.Z, self.X, Guf)
        return {k: -g for k, g in out.items()}

    def predict_f(self, xs, diag=True):
        """sparse_gpr.py:155-195 (+ the constant mean)."""
        xs = xr.ld(xs)
        t1 = xr.solve_lower(self.L, xr.expr_K(self.spec, self.Z, xs))
        t2 = xr.solve_lower(self.LB, t1)
        mean = t2.T @ self.c + self.mean
        if diag:
            return mean, np.repeat((xr.expr_Kdiag(self.spec, xs) - np.sum(t1 * t1, 0) + np.sum(t2 * t2, 0))[:, None], self.p, 1)
        return mean, xr.expr_K(self.spec, xs, None) + t2.T @ t2 - t1.T @ t1


# ---------------------------------------------------------------------------------------------------------------------
# SVGP
# ---------------------------------------------------------------------------------------------------------------------
class SVGPRef:
    """x, y: the rows of ONE evaluation (a minibatch: the gathered rows); num_data: rows of the whole data set."""

    def __init__(self, x, y, z, kernel, noise, q_mu, q_sqrt, mean=None, num_data=None, plant=None):
        self.X, self.Y, self.Z = xr.ld(x), xr.ld(y), xr.ld(z)
        self.n, self.dy = self.Y.shape
        self.m = self.Z.shape[0]
        self.spec = spec_of(kernel, self.X.shape[1]) if isinstance(kernel, dict) else kernel
        self.s = LD(noise)
        self.q_mu, self.S_L = xr.ld(q_mu), np.tril(xr.ld(q_sqrt))
        self.mean = np.zeros(self.dy, dtype=LD) if mean is None else xr.ld(mean)
        if plant not in (None, "scale_one", "gq_triangle", "drop_kd_diag"):
            raise ValueError(plant)
        self.plant = plant
        self.scale = LD(1) if plant == "scale_one" else LD(self.n if num_data is None else num_data) / self.n
        self.Kuu = xr.expr_K(self.spec, self.Z, None)
        self.L = xr.cholesky(self.Kuu)
        self.beta = xr.solve_lower(self.L, self.S_L)
        self.w = xr.solve_lower(self.L, self.q_mu)
        self.f_mean, self.f_var = self.marginals(self.X)

    def marginals(self, a, full=False):
        """sparse_gpr.py:358-377: (mean [n, dy], variance [n] or covariance [n, n]) of q(f) at the rows of a."""
        a = xr.ld(a)
        alpha = xr.solve_lower(self.L, xr.expr_K(self.spec, self.Z, a)).T
        mean = alpha @ self.w + self.mean
        gamma = alpha @ self.beta
        if full:
            return mean, xr.expr_K(self.spec, a, None) - alpha @ alpha.T + gamma @ gamma.T
        return mean, xr.expr_Kdiag(self.spec, a) - np.sum(alpha * alpha, 1) + np.sum(gamma * gamma, 1)

    def kl(self):
        return (LD(0.5) * self.dy * (np.sum(self.beta ** 2) - self.m + 2 * np.sum(np.log(np.diag(self.L))) - 2 * np.sum(np.log(np.diag(self.S_L))))
                + LD(0.5) * np.sum(self.w ** 2))

    def data_term(self):
        """sum over rows and output columns of E_q[log N(y | f, s)], times num_data / rows."""
        n, dy, s = self.n, self.dy, self.s
        return self.scale * -LD(0.5) * (n * dy * (LOG2PI + np.log(s)) + (np.sum((self.Y - self.f_mean) ** 2) + dy * np.sum(self.f_var)) / s)

    def bound(self):
        return self.data_term() - self.kl()

    def loss(self):
        return -self.bound()

    def loss_grads(self, with_Z=True):
        """-> {variance, length_scales (composite: + linear_variance, constant), noise, mean, Z, q_mu, q_sqrt}: d loss / d raw.

        The bound as a function of the whitened quantities alpha = (L^-1 Kuf)^T, w = L^-1 q_mu, beta = L^-1 S_L (Qm = beta beta^T - I):
            f_mean = alpha w + mean,   f_var_i = Kdiag_i + alpha_i Qm alpha_i^T
            KL = dy/2 (|beta|^2 - M + 2 sum log L_ii - 2 sum log S_L,ii) + 1/2 |w|^2
        with upstream g_mean = c (y - f_mean)/s, g_var = -c dy/(2s) per row (c = num_data / rows), G_Q = alpha^T diag(g_var) alpha:
            G_alpha = g_mean w^T + diag(g_var) alpha (Qm + Qm^T),   G_w = alpha^T g_mean - w,   G_beta = (G_Q + G_Q^T) beta - dy beta
        and each solve X = L^-1 Y pulled back: dY = L^-T G_X, and onto L through dX = -Phi(W) X, W = L^-1 dKuu L^-T, Phi = lower
        triangle with half the diagonal.  With T = G_alpha^T alpha + G_w w^T + G_beta beta^T (NOT assumed symmetric) that is
        dF = -sum(T * Phi(W)) = -tr(Psi(T) W), Psi(T) = 1/2 (strict lower + its mirror + diagonal); KL's sum log L_ii adds
        -dy/2 tr W.  So dKuu = -L^-T (Psi(T) + dy/2 I) L^-1, dKuf = L^-T G_alpha^T, dq_mu = L^-T G_w,
        dS_L = tril(L^-T G_beta) + dy / diag(S_L) on the diagonal, dKdiag = g_var."""
        n, dy, m, s, c = self.n, self.dy, self.m, self.s, self.scale
        Li = xr.solve_lower(self.L, np.eye(m, dtype=LD))
        alpha = xr.solve_lower(self.L, xr.expr_K(self.spec, self.Z, self.X)).T
        Qm = self.beta @ self.beta.T - np.eye(m, dtype=LD)
        g_mean = c * (self.Y - self.f_mean) / s
        g_var = np.full(n, -c * dy / (2 * s), dtype=LD)
        GQ = (alpha.T * g_var) @ alpha
        if self.plant == "gq_triangle":
            GQ = np.tril(GQ)
        G_alpha = g_mean @ self.w.T + (alpha * g_var[:, None]) @ (Qm + Qm.T)
        G_w = alpha.T @ g_mean - self.w
        G_beta = (GQ + GQ.T) @ self.beta - dy * self.beta
        T = G_alpha.T @ alpha + G_w @ self.w.T + G_beta @ self.beta.T
        Psi = LD(0.5) * (np.tril(T, -1) + np.tril(T, -1).T + np.diag(np.diag(T)))
        dKuu = -Li.T @ (Psi + LD(0.5) * dy * np.eye(m, dtype=LD)) @ Li
        dKuf = Li.T @ G_alpha.T
        dSL = np.tril(Li.T @ G_beta)
        if self.plant != "drop_kd_diag":
            dSL[np.diag_indices(m)] += dy / np.diag(self.S_L)
        raw_S = np.tril(dSL, -1) + np.diag(np.diag(dSL) * np.diag(self.S_L))
        resid = np.sum((self.Y - self.f_mean) ** 2) + dy * np.sum(self.f_var)
        g_s = c * (-LD(0.5) * n * dy / s + LD(0.5) * resid / (s * s))
        out = _kernel_grads(self.spec, [(self.Z, None, dKuu), (self.Z, self.X, dKuf)], [(self.X, g_var)])
        out["noise"] = np.array([s * g_s])
        out["mean"] = g_mean.sum(0)
        out["q_mu"] = Li.T @ G_w
        out["q_sqrt"] = raw_S
        if with_Z:
            out["Z"] = point_grads(self.spec, self.Z, None, dKuu) + point_grads(self.spec, self.Z, self.X, dKuf)
        return {k: -g for k, g in out.items()}

    def predict_f(self, xs, diag=True):
        mean, v = self.marginals(xs, full=not diag)
        return mean, (np.repeat(v[:, None], self.dy, 1) if diag else v)


# ---------------------------------------------------------------------------------------------------------------------
# FITC
# ---------------------------------------------------------------------------------------------------------------------
FITC_PLANTS = ("drop_last_row", "sums_first_chunk", "aga_triangle", "drop_kdiag_grad", "g_without_h")


class FITCRef:
    """the F of gptorch_amd/models/_fitc.py's header, whitened: A = L^-1 Kuf, lambda = Kdiag - colsum(A^2) + s,
    B = I + A D A^T (D = diag(1 / lambda)), c = LB^-1 A D err."""

    def __init__(self, x, y, z, kernel, noise, mean=None, jitter=0.0, plant=None, plant_at=0):
        self.X, self.Y, self.Z = xr.ld(x), xr.ld(y), xr.ld(z)
        self.n, self.p = self.Y.shape
        self.m = self.Z.shape[0]
        self.spec = spec_of(kernel, self.X.shape[1]) if isinstance(kernel, dict) else kernel
        self.s = LD(noise)
        self.mean = np.zeros(self.p, dtype=LD) if mean is None else xr.ld(mean)
        self.err = self.Y - self.mean
        if plant is not None and plant not in FITC_PLANTS:
            raise ValueError(plant)
        self.plant = plant
        # mask_c: the columns of A that enter A D A^T and A D err; mask_s: the rows counted in sum log lambda and sum err^2 / lambda
        self.mask_c, self.mask_s = np.ones(self.n, dtype=LD), np.ones(self.n, dtype=LD)
        if plant == "drop_last_row":
            self.mask_c[-1] = 0
        elif plant == "sums_first_chunk":
            self.mask_s[plant_at:] = 0
        self.Kuu = xr.expr_K(self.spec, self.Z, None) + LD(jitter) * np.eye(self.m, dtype=LD)
        self.Kuf = xr.expr_K(self.spec, self.Z, self.X)
        self.L = xr.cholesky(self.Kuu)
        self.A = xr.solve_lower(self.L, self.Kuf)
        self.lam = xr.expr_Kdiag(self.spec, self.X) - np.sum(self.A * self.A, 0) + self.s
        self.Ac = self.A * self.mask_c
        self.B = np.eye(self.m, dtype=LD) + (self.Ac / self.lam) @ self.Ac.T
        self.LB = xr.cholesky(self.B)
        self.b = (self.Ac / self.lam) @ self.err
        self.c = xr.solve_lower(self.LB, self.b)

    def lml(self):
        n, p = self.n, self.p
        return (-LD(0.5) * p * n * LOG2PI - LD(0.5) * p * np.sum(self.mask_s * np.log(self.lam)) - p * np.sum(np.log(np.diag(self.LB)))
                - LD(0.5) * np.sum(self.mask_s * np.sum(self.err ** 2, 1) / self.lam) + LD(0.5) * np.sum(self.c ** 2))

    def loss(self):
        return -self.lml()

    def loss_grads(self, with_Z=True):
        """-> {variance, length_scales (composite: + linear_variance, constant), noise, mean, Z}: d loss / d raw.

        F as a function of (A_c, lambda, err), A_c the columns of A that enter B and b (all of them unless planted), beta = B^-1 b,
        q_i = A_c,i^T beta, h_i = A_c,i^T B^-1 A_c,i, from dB = dA_c D A_c^T + A_c D dA_c^T + A_c dD A_c^T, db = dA_c D err + A_c dD err:
            dF/dA_c      = [beta (err - A_c^T beta)^T - p B^-1 A_c] D                                    (lambda held fixed)
            dF/dlambda_i = -p/(2 lambda_i) + p h_i/(2 lambda_i^2) + (|err_i|^2 - 2 q_i.err_i + |q_i|^2)/(2 lambda_i^2)   (= g_i / 2)
            dF/derr_i    = -(err_i - q_i)/lambda_i
        lambda_i = Kdiag_i - |a_i|^2 + s hands dF/dlambda on: dF/dKdiag_i = dF/dlambda_i, dF/ds = their sum, and -2 A diag(dF/dlambda)
        joins dF/dA_c in G_A (M x N).  A = L^-1 Kuf is pulled back as in VFERef.loss_grads: dKuf = L^-T G_A and, with T = G_A A^T formed
        as it stands, dKuu = -L^-T Psi(T) L^-1, Psi(T) = 1/2 (strict lower + its mirror + diagonal)."""
        n, p, m, s, lam = self.n, self.p, self.m, self.s, self.lam
        eye = np.eye(m, dtype=LD)
        Li = xr.solve_lower(self.L, eye)
        Binv = _inverse_from_factor(self.LB)[1]
        A, Ac, mc, ms = self.A, self.Ac, self.mask_c, self.mask_s
        beta = Binv @ self.b
        q = Ac.T @ beta                                                    # [n, p]
        h = np.sum(Ac * (Binv @ Ac), 0)
        if self.plant == "g_without_h":
            h = np.zeros(n, dtype=LD)
        g_lam = (-LD(0.5) * p * ms / lam + LD(0.5) * p * h / lam ** 2
                 + LD(0.5) * (ms * np.sum(self.err ** 2, 1) - 2 * np.sum(q * self.err, 1) + np.sum(q * q, 1)) / lam ** 2)
        GA_c = ((beta @ (self.err - q).T - p * (Binv @ Ac)) / lam) * mc
        GA_lam = -2 * A * g_lam
        GA = GA_c + GA_lam
        psi = lambda T: LD(0.5) * (np.tril(T, -1) + np.tril(T, -1).T + np.diag(np.diag(T)))
        if self.plant == "aga_triangle":
            Psi = psi(GA_c @ A.T) + LD(0.5) * np.tril(GA_lam @ A.T)
        else:
            Psi = psi(GA @ A.T)
        Guu = -Li.T @ Psi @ Li
        Guf = Li.T @ GA
        g_err = -(ms[:, None] * self.err - q) / lam[:, None]
        g_kd = np.zeros(n, dtype=LD) if self.plant == "drop_kdiag_grad" else g_lam
        out = _kernel_grads(self.spec, [(self.Z, None, Guu), (self.Z, self.X, Guf)], [(self.X, g_kd)])
        out["noise"] = np.array([s * np.sum(g_lam)])
        out["mean"] = -g_err.sum(0)
        if with_Z:
            out["Z"] = point_grads(self.spec, self.Z, None, Guu) + point_grads(self.spec, self.Z, self.X, Guf)
        return {k: -g for k, g in out.items()}

    def predict_f(self, xs, diag=True):
        """the collapsed equations of _fitc.py _predict (+ the constant mean)."""
        xs = xr.ld(xs)
        t1 = xr.solve_lower(self.L, xr.expr_K(self.spec, self.Z, xs))
        t2 = xr.solve_lower(self.LB, t1)
        mean = t2.T @ self.c + self.mean
        if diag:
            return mean, np.repeat((xr.expr_Kdiag(self.spec, xs) - np.sum(t1 * t1, 0) + np.sum(t2 * t2, 0))[:, None], self.p, 1)
        return mean, xr.expr_K(self.spec, xs, None) + t2.T @ t2 - t1.T @ t1


# ---------------------------------------------------------------------------------------------------------------------
# the plain fp64 evaluations behind e64
# ---------------------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64)).clone()


def _raw_leaves(spec):
    return {l["id"]: xr.leaf_tensors(l, log=True, grad=True) for l in xr.spec_leaves(spec)}


def _direct_K(spec, raw, a, b=None):
    return xr.direct_expr_K(spec, a, b, {i: (v.exp(), None if l is None else l.exp()) for i, (v, l) in raw.items()})


def _direct_Kdiag(spec, raw, a):
    total = 0.0
    for g in spec:
        prod = 1.0
        for l in g:
            v = raw[l["id"]][0].exp()
            prod = prod * ((a * a * v).sum(1) if l["type"] == "linear" else v.expand(a.shape[0]))
        total = total + prod
    return total


def _named(raw, grads_of):
    out = {}
    for i, (v, l) in raw.items():
        if i == "k":
            out["variance"], out["length_scales"] = grads_of(v), grads_of(l)
        else:
            out[i] = grads_of(v)
    return out


def _grad_np(t):
    return np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy().copy()


class Direct64VFE(xr.DirectVFE):
    """xr.DirectVFE (orc.VFEOracle's op chain in fp64, K by direct differences) for any spec, with the constant mean and the
    jitter VFERef takes, parameters as raw autograd leaves."""

    def __init__(self, x, y, z, kernel, noise, mean=None, jitter=0.0):
        self.X, self.Ydata, self.Z = _t(x), _t(y), _t(z).requires_grad_(True)
        self.spec = spec_of(kernel, self.X.shape[1]) if isinstance(kernel, dict) else kernel
        self.raw = _raw_leaves(self.spec)
        self.raw_noise = torch.tensor([math.log(noise)], dtype=torch.float64, requires_grad=True)
        self.mean_val = (torch.zeros(self.Ydata.shape[1], dtype=torch.float64) if mean is None else _t(mean)).requires_grad_(True)
        self.jitter = float(jitter)

    noise = property(lambda self: self.raw_noise.exp())
    Y = property(lambda self: self.Ydata - self.mean_val)                   # the `err` of VFEOracle._common

    def K(self, a, b=None):
        Km = _direct_K(self.spec, self.raw, a, b)
        if b is None and a is self.Z and self.jitter:
            Km = Km + self.jitter * torch.eye(a.shape[0], dtype=torch.float64)
        return Km

    def log_likelihood(self):
        """orc.VFEOracle.log_likelihood with this kernel's diagonal."""
        n, p = self.Ydata.shape
        L, A, AAT, LB, c = self._common(self.X)
        err = self.Y
        elbo = -0.5 * p * n * math.log(2 * math.pi) - p * LB.diag().log().sum() - 0.5 * p * n * self.noise.log()
        elbo = elbo - 0.5 * (err.pow(2).sum() + p * _direct_Kdiag(self.spec, self.raw, self.X).sum()) / self.noise
        return (elbo + 0.5 * c.pow(2).sum() + 0.5 * p * AAT.diag().sum())[0]

    def loss_and_grads(self):
        leaves = [t for pair in self.raw.values() for t in pair if t is not None] + [self.raw_noise, self.mean_val, self.Z]
        for t in leaves:
            t.grad = None
        loss = -self.log_likelihood()
        loss.backward()
        out = _named(self.raw, _grad_np)
        out.update(noise=_grad_np(self.raw_noise), mean=_grad_np(self.mean_val), Z=_grad_np(self.Z))
        return loss.item(), out

    def predict_f(self, x_new, diag=True):
        with torch.no_grad():
            xs = _t(x_new)
            L, A, AAT, LB, c = self._common(self.X)
            t1 = orc.trtrs(self.K(self.Z, xs), L)
            t2 = orc.trtrs(t1, LB)
            mean = t2.t() @ c + self.mean_val
            if diag:
                v = _direct_Kdiag(self.spec, self.raw, xs) - t1.pow(2).sum(0) + t2.pow(2).sum(0)
                return mean.numpy(), v[:, None].expand_as(mean).numpy()
            return mean.numpy(), (self.K(xs) + t2.t() @ t2 - t1.t() @ t1).numpy()


class Direct64FITC(Direct64VFE):
    """the M-sized (Woodbury) fp64 evaluation of FITC (tests/_fitc_oracle.FITCOracle.woodbury_lml) with Direct64VFE's leaves and
    its K by direct differences; gradients by autograd (Direct64VFE.loss_and_grads)."""

    def _inputs(self):
        return self.K(self.Z), self.K(self.Z, self.X), _direct_Kdiag(self.spec, self.raw, self.X), self.noise, self.Y

    def log_likelihood(self):
        return fo.FITCOracle.woodbury_lml(*self._inputs()).reshape(())

    def predict_f(self, x_new, diag=True):
        with torch.no_grad():
            xs = _t(x_new)
            Kuu, Kuf, Kd, s2, err = self._inputs()
            L = torch.linalg.cholesky(Kuu)
            A = orc.trtrs(Kuf, L)
            lam = Kd - A.pow(2).sum(0) + s2
            LB = torch.linalg.cholesky(torch.eye(Kuu.shape[0], dtype=torch.float64) + (A / lam) @ A.t())
            c = orc.trtrs((A / lam) @ err, LB)
            t1 = orc.trtrs(self.K(self.Z, xs), L)
            t2 = orc.trtrs(t1, LB)
            mean = t2.t() @ c + self.mean_val
            if diag:
                v = _direct_Kdiag(self.spec, self.raw, xs) - t1.pow(2).sum(0) + t2.pow(2).sum(0)
                return mean.numpy(), v[:, None].expand_as(mean).numpy()
            return mean.numpy(), (self.K(xs) + t2.t() @ t2 - t1.t() @ t1).numpy()


class Direct64SVGP(so.SVGPOracle):
    """tests/_svgp_oracle.SVGPOracle with its K by direct differences: only the arithmetic differs from SVGPRef."""

    def K(self, a, b=None):
        var, ls = self.raw["variance"].exp(), self.raw["length_scales"].exp()
        if self.kind == COMPOSITE:
            rows, cols = a.shape[0], (a if b is None else b).shape[0]
            return orc.linear_K(a, b, self.raw["linear_variance"].exp()) + xr.direct_kernel_K("Rbf", a, b, var, ls) \
                + self.raw["constant"].exp().expand(rows, cols)
        return xr.direct_kernel_K(self.kind, a, b, var, ls)


# ---------------------------------------------------------------------------------------------------------------------
# one case -> reference values and e64
# ---------------------------------------------------------------------------------------------------------------------
def e64_of(loss64, grads64, pred64, loss_ld, grads_ld, pred_ld):
    """the distances tests/_xref.tol scales: loss and every gradient relative to max(1, |reference|), predictions absolute.
    pred*: (mean, var, cov)."""
    e = dict(loss=xr.rel_err(loss64, loss_ld), mean=xr.abs_err(pred64[0], pred_ld[0]),
             var=max(xr.abs_err(pred64[1], pred_ld[1]), xr.abs_err(pred64[2], pred_ld[2])))
    e["grads"] = {k: xr.rel_err(np.asarray(grads64[k]).reshape(np.shape(g)), g) for k, g in grads_ld.items() if k in grads64}
    e["grad"] = max(e["grads"].values()) if e["grads"] else 0.0
    return e


def evaluate(ref, d64, xs, with_Z=True, **kw):
    """-> dict(loss, grads, mean, var, cov, e64) of a VFERef / SVGPRef and its Direct64 twin (gradients: those both have;
    kw: what the twin's loss_and_grads takes, e.g. idx= of a minibatch)."""
    grads = ref.loss_grads(with_Z=with_Z)
    mean, var = ref.predict_f(xs, True)
    _, cov = ref.predict_f(xs, False)
    loss64, grads64 = d64.loss_and_grads(**kw)
    m64, v64 = d64.predict_f(xs, True)
    _, c64 = d64.predict_f(xs, False)
    grads = {k: g for k, g in grads.items() if k in grads64}
    v64 = v64 if np.ndim(v64) == 2 else np.repeat(np.asarray(v64)[:, None], mean.shape[1], 1)
    return dict(loss=ref.loss(), grads=grads, mean=mean, var=var, cov=cov,
                e64=e64_of(loss64, grads64, (m64, v64, c64), ref.loss(), grads, (mean, var, cov)))


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_sparse_ref_host.py and tests/test_gpu_sparse_xref.py
# ---------------------------------------------------------------------------------------------------------------------
# knobs: the settings of gptorch_amd.models.sparse_gpr one run of the case is made under (every set against the SAME reference)
_M52 = dict(kind="Matern52", variance=1.2, length_scales=0.9)
_COMP = dict(kind=COMPOSITE, linear_variance=0.3, variance=1.1, length_scales=0.8, constant=0.5)
VFE_CASES = [
    dict(name="one_chunk", n=300, m=40, d=1, dy=1, kernel=dict(kind="Exp", variance=1.1, length_scales=0.6), noise=0.05, seed=301, knobs=[{}]),
    # (VFE takes no mean function -- sparse_gpr.py:125 uses y itself as the residual -- so this case runs without the Constant mean;
    # VFERef's mean gradient is held by the host tests alone)
    dict(name="m_across_a_leaf", n=700, m=129, d=3, dy=2, kernel=dict(kind="Matern52", variance=1.2, length_scales=[0.8, 1.0, 1.2], ARD=True),
         noise=0.05, seed=311, knobs=[{}]),
    dict(name="ragged_multi_chunk", n=1300, m=130, d=3, dy=5, kernel=dict(kind="Rbf", variance=1.1, length_scales=[0.5, 0.6, 0.7], ARD=True),
         noise=0.1, seed=321, knobs=[dict(CHUNK_ROWS=256, LANES=1), dict(CHUNK_ROWS=256, LANES=2)], chunks=[256] * 5 + [20]),
    dict(name="exact_multiple", n=1024, m=64, d=2, dy=1, kernel=dict(kind="Matern32", variance=1.3, length_scales=0.8), noise=0.05, seed=331,
         knobs=[dict(CHUNK_ROWS=256)], chunks=[256] * 4),
    dict(name="short_k_slices", n=1300, m=130, d=3, dy=1, kernel=_M52, noise=0.05, seed=341,
         knobs=[dict(CHUNK_ROWS=512, SYRK_K_SLICE=128), dict(CHUNK_ROWS=512, SYRK_K_SLICE=0)], chunks=[512, 512, 276]),
    dict(name="split_k_tail", n=8592, m=130, d=3, dy=2, kernel=dict(kind="Matern32", variance=1.3, length_scales=0.9), noise=0.05, seed=351,
         knobs=[dict(CHUNK_ROWS=8192, SPLIT_K=2)], chunks=[8192, 400]),
    # kp % (16 * split) != 0 with split > 1: as ONE chunk of 8200 rows (CHUNK_ROWS = 8320: the sequential branch writes parts[0] with
    # beta = 0 and parts[1] stays zero) and as 8192 + 8 rows (CHUNK_ROWS = 8192: batched partials, then a 16-column tail)
    dict(name="split_k_miss", n=8200, m=130, d=3, dy=1, kernel=_M52, noise=0.05, seed=361,
         knobs=[dict(CHUNK_ROWS=8320, SPLIT_K=2), dict(CHUNK_ROWS=8192, SPLIT_K=2)]),
    dict(name="inverse_form", n=600, m=130, d=2, dy=1, kernel=dict(kind="Rbf", variance=1.1, length_scales=0.35), noise=0.1, seed=371,
         knobs=[dict(INVERSE_MIN_M=128, INVERSE_BLOCK=48, CHUNK_ROWS=256)], chunks=[256, 256, 88]),
    dict(name="blocked_one_block", n=700, m=130, d=3, dy=2, kernel=_M52, noise=0.05, seed=381,
         knobs=[dict(BLOCKED_SOLVE_MIN_M=128, CHUNK_ROWS=256)], chunks=[256, 256, 188]),
    dict(name="blocked_two_blocks", n=4700, m=1153, d=3, dy=1, kernel=dict(kind="Matern52", variance=1.2, length_scales=0.7), noise=0.05, seed=391,
         knobs=[dict(BLOCKED_SOLVE_MIN_M=1024, CHUNK_ROWS=2048)], chunks=[2048, 2048, 604], golden=True),
    dict(name="composite", n=500, m=48, d=3, dy=1, kernel=_COMP, noise=0.08, seed=401, knobs=[dict(CHUNK_ROWS=256)], chunks=[256, 244]),
    dict(name="ladder", n=400, m=40, d=2, dy=1, kernel=dict(kind="Rbf", variance=1.1, length_scales=0.8), noise=0.05, seed=411, knobs=[{}],
         ladder=True),
]
# FITC: kernel hyper-parameters, noise and seeds of the VFE rows of the same name (new seeds where there is none); `mean`: a
# Constant mean function.  inverse_knob_ignored: a hooked evaluation never takes the inverse form, whatever INVERSE_MIN_M says.
FITC_CASES = [
    dict(name="one_chunk", n=300, m=40, d=1, dy=1, kernel=dict(kind="Exp", variance=1.1, length_scales=0.6), noise=0.05, seed=301, knobs=[{}]),
    dict(name="m_odd_across_a_leaf", n=700, m=129, d=3, dy=2, kernel=dict(kind="Matern52", variance=1.2, length_scales=[0.8, 1.0, 1.2], ARD=True),
         noise=0.05, mean=[0.3, -0.2], seed=601, knobs=[{}]),
    dict(name="dy_across_16", n=200, m=33, d=2, dy=17, kernel=dict(kind="Matern32", variance=1.3, length_scales=0.8), noise=0.05,
         mean=[0.3, -0.2, 0.1, 0.0, 0.25, -0.4, 0.15, 0.05, -0.1, 0.2, -0.3, 0.35, -0.15, 0.45, -0.05, 0.4, -0.25], seed=611, knobs=[{}]),
    dict(name="ragged_multi_chunk", n=1300, m=130, d=3, dy=5, kernel=dict(kind="Rbf", variance=1.1, length_scales=[0.5, 0.6, 0.7], ARD=True),
         noise=0.1, seed=321, knobs=[dict(CHUNK_ROWS=256, LANES=1), dict(CHUNK_ROWS=256, LANES=2)], chunks=[256] * 5 + [20]),
    dict(name="exact_multiple", n=1024, m=64, d=2, dy=1, kernel=dict(kind="Matern32", variance=1.3, length_scales=0.8), noise=0.05, seed=331,
         knobs=[dict(CHUNK_ROWS=256)], chunks=[256] * 4),
    dict(name="short_k_slices", n=1300, m=130, d=3, dy=1, kernel=_M52, noise=0.05, seed=341,
         knobs=[dict(CHUNK_ROWS=512, SYRK_K_SLICE=128), dict(CHUNK_ROWS=512, SYRK_K_SLICE=0)], chunks=[512, 512, 276]),
    dict(name="split_k_tail", n=8592, m=130, d=3, dy=2, kernel=dict(kind="Matern32", variance=1.3, length_scales=0.9), noise=0.05, seed=351,
         knobs=[dict(CHUNK_ROWS=8192, SPLIT_K=2)], chunks=[8192, 400]),
    dict(name="split_k_miss", n=8200, m=130, d=3, dy=1, kernel=_M52, noise=0.05, seed=361,
         knobs=[dict(CHUNK_ROWS=8320, SPLIT_K=2), dict(CHUNK_ROWS=8192, SPLIT_K=2)]),
    dict(name="blocked_one_block", n=700, m=130, d=3, dy=2, kernel=_M52, noise=0.05, seed=381,
         knobs=[dict(BLOCKED_SOLVE_MIN_M=128, CHUNK_ROWS=256)], chunks=[256, 256, 188]),
    dict(name="blocked_two_blocks", n=4700, m=1153, d=3, dy=1, kernel=dict(kind="Matern52", variance=1.2, length_scales=0.7), noise=0.05, seed=391,
         knobs=[dict(BLOCKED_SOLVE_MIN_M=1024, CHUNK_ROWS=2048)], chunks=[2048, 2048, 604], golden=True),
    dict(name="composite", n=500, m=48, d=3, dy=1, kernel=_COMP, noise=0.08, seed=401,
         knobs=[dict(CHUNK_ROWS=256, LANES=1), dict(CHUNK_ROWS=256, LANES=2)], chunks=[256, 244]),
    # (cond K(Z) ~ 1e8, as VFE's inverse_form: the one case besides the ladder whose tolerances stand above the floors.  Seeds 621,
    # 631 and 641 put d/dZ's e64 at 5e-9 and more, 16 e64 at or over the host tests' cap of 1e-7; 651 leaves it 2.8x under)
    dict(name="inverse_knob_ignored", n=600, m=130, d=2, dy=1, kernel=dict(kind="Rbf", variance=1.1, length_scales=0.35), noise=0.1, seed=651,
         knobs=[dict(INVERSE_MIN_M=128, CHUNK_ROWS=256)], chunks=[256, 256, 88]),
    dict(name="ladder", n=400, m=40, d=2, dy=1, kernel=dict(kind="Rbf", variance=1.1, length_scales=0.8), noise=0.05, seed=411, knobs=[{}],
         ladder=True),
]
SVGP_CASES = [
    dict(name="small", n=37, m=5, d=1, dy=1, kernel=dict(kind="Exp", variance=1.1, length_scales=0.6), noise=0.1, seed=501, knobs=[{}]),
    dict(name="dy9", n=130, m=40, d=3, dy=9, kernel=dict(kind="Matern52", variance=1.2, length_scales=[0.8, 1.0, 1.2], ARD=True), noise=0.05,
         mean=[0.3, -0.2, 0.1, 0.0, 0.25, -0.4, 0.15, 0.05, -0.1], seed=511, knobs=[{}]),
    dict(name="saved_vs_recompute", n=1300, m=129, d=3, dy=2, kernel=dict(kind="Rbf", variance=1.1, length_scales=0.6), noise=0.1, seed=521,
         knobs=[{}, dict(CHUNK_ROWS=256)]),
    dict(name="minibatch", n=1000, m=64, d=2, dy=1, kernel=dict(kind="Matern32", variance=1.3, length_scales=0.8), noise=0.05, seed=531, nb=192,
         knobs=[{}]),
    dict(name="composite", n=500, m=48, d=3, dy=1, kernel=_COMP, noise=0.08, seed=541, knobs=[dict(CHUNK_ROWS=256)]),
]


def case_inputs(case, svgp=False):
    """-> dict(x, y, z, xs [, q_mu, q_sqrt, idx]): rng.make_regression, a quarter of Z on rows of x (Exp's cusp in Kuf), the rest of Z
    standard normal like x; xs: 12 fresh points and 4 training rows (which are inducing points too)."""
    from gptorch_amd import rng
    n, m, d, dy, seed = case["n"], case["m"], case["d"], case["dy"], case["seed"]
    x, y = rng.make_regression(n, d, dy, seed=seed)
    z = np.concatenate([x[:m // 4], rng.normal(seed + 2, (m - m // 4, d))])
    if case.get("ladder"):
        z[-1] = z[-2]                                                       # two identical inducing points: K(Z) is singular
    out = dict(x=x, y=y, z=z, xs=np.concatenate([rng.normal(seed + 3, (12, d)), x[:4]]), idx=None)
    if svgp:
        q = so.case_inputs(dict(case, seed_x=seed, seed_z=seed + 2, seed_q=seed + 4, seed_xs=seed + 3, seed_idx=seed + 6), z=z)
        out.update(q_mu=q["q_mu"], q_sqrt=q["q_sqrt"], idx=None if q["idx"] is None else np.sort(q["idx"]))
    return out


def vfe_refs(case, inp, jitter=0.0, **plant):
    return (VFERef(inp["x"], inp["y"], inp["z"], case["kernel"], case["noise"], jitter=jitter, **plant),
            Direct64VFE(inp["x"], inp["y"], inp["z"], case["kernel"], case["noise"], jitter=jitter))


def svgp_refs(case, inp, **plant):
    """(SVGPRef on the rows of the evaluation, Direct64SVGP on the whole data set -- evaluate it with idx=inp["idx"])."""
    i = slice(None) if inp["idx"] is None else inp["idx"]
    return (SVGPRef(inp["x"][i], inp["y"][i], inp["z"], case["kernel"], case["noise"], inp["q_mu"], inp["q_sqrt"], mean=case.get("mean"),
                    num_data=case["n"], **plant),
            Direct64SVGP(inp["x"], inp["y"], inp["z"], case["kernel"], noise=case["noise"], q_mu=inp["q_mu"], q_sqrt=inp["q_sqrt"],
                         mean=case.get("mean")))


def fitc_refs(case, inp, jitter=0.0, **plant):
    return (FITCRef(inp["x"], inp["y"], inp["z"], case["kernel"], case["noise"], mean=case.get("mean"), jitter=jitter, **plant),
            Direct64FITC(inp["x"], inp["y"], inp["z"], case["kernel"], case["noise"], mean=case.get("mean"), jitter=jitter))


def fitc_reference(case, inp, jitter=0.0):
    ref, d64 = fitc_refs(case, inp, jitter)
    return evaluate(ref, d64, inp["xs"], with_Z=True)


def vfe_reference(case, inp, jitter=0.0):
    ref, d64 = vfe_refs(case, inp, jitter)
    return evaluate(ref, d64, inp["xs"], with_Z=True)


def svgp_reference(case, inp):
    ref, d64 = svgp_refs(case, inp)
    return evaluate(ref, d64, inp["xs"], idx=inp["idx"])
