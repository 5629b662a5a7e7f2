"""
TEST INFRASTRUCTURE ONLY -- leave-one-out cross-validation of the exact GP (Rasmussen & Williams 5.4.2, eqs. 5.10-5.13), stated
twice on the host: in numpy's long double on top of tests/_xref.GPRRef (LooRef), and in plain fp64 (LooTorch: torch, a dense
LAPACK inverse, gradients by autograd; loo_terms / loo_G with dtype=np.float64: the same sums in numpy fp64).  With P = Kyy^-1, r = Y - m, a = P r, p = diag P:

    y_i - mu_i = q_i = a_i / p_i        sigma_i^2 = 1 / p_i                 (the predictive of the OBSERVATION y_i given y_-i)
    L_LOO = sum_i [1/2 dy log p_i - 1/2 sum_c a_ic q_ic] - 1/2 n dy log 2 pi
    d_i = dy / (2 p_i) + sum_c a_ic^2 / (2 p_i^2),  w = P q,  Q = P diag(d) P
    dL_LOO/dtheta = sum_ij G_ij dKyy_ij/dtheta,  G = -Q + 1/2 (a w^T + w a^T),  dL_LOO/dnoise = tr G,  dL_LOO/dr = -w

LooRef.refit(i) does NOT use any of this: it deletes row i, factorises the remaining n - 1 points and predicts y_i.

gptorch_amd never imports this module.
"""
import numpy as np
import torch

from tests import _xref as xr

LD = xr.LD
U = 2.0 ** -53


def loo_terms(p, a, dtype=LD):
    """per point, from p = diag(P) [n] and a = P r [n, dy]: (q [n, dy], var [n], d [n], L_LOO) in `dtype`."""
    p, a = np.asarray(p, dtype=dtype), np.asarray(a, dtype=dtype)
    n, dy = a.shape
    q = a / p[:, None]
    d = dy / (2 * p) + np.sum(a * a, 1) / (2 * p * p)
    terms = dtype(0.5) * (dy * np.log(p) - np.sum(a * q, 1))
    value = np.sum(terms) - dtype(0.5) * n * dy * np.log(2 * dtype(np.pi))
    return q, 1 / p, d, value, terms


def loo_G(P, a, dtype=LD):
    """(G [n, n], w [n, dy]) from the full symmetric P and a."""
    P, a = np.asarray(P, dtype=dtype), np.asarray(a, dtype=dtype)
    q, _, d, _, _ = loo_terms(np.diag(P), a, dtype)
    w = P @ q
    Q = (P * d[None, :]) @ P
    return -Q + dtype(0.5) * (a @ w.T + w @ a.T), w


class LooRef(xr.GPRRef):
    """GPRRef plus the leave-one-out closed form, every intermediate in long double."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        Li = xr.solve_lower(self.L, np.eye(self.n, dtype=LD))
        self.P = np.einsum("ki,kj->ij", Li, Li)
        self.a = xr.solve_upper_t(self.L, self.alpha)
        self.q, self.s2, self.d, self.value, _ = loo_terms(np.diag(self.P), self.a)

    def loo(self):
        return self.value

    def loss(self):
        return -self.value

    def loo_predict(self):
        return self.Y - self.q, np.repeat(self.s2[:, None], self.dy, 1)

    def G(self):
        return loo_G(self.P, self.a)

    def loss_grads(self):
        """d(-L_LOO) / d(log variance, log ell [d or 1], log noise, mean [dy]), as GPRRef.loss_grads orders them."""
        G, w = self.G()
        g_var, g_ls = xr.kernel_param_grads(self.kind, self.X, None, self.var, self.ls, G, self.ARD)
        return [-g_var, -g_ls, -np.array([self.noise * np.trace(G)]), -w.sum(0)]

    def refit(self, i):
        """(mean [dy], variance) of y_i from a model that never saw point i: a fresh GPRRef on the other n - 1 rows."""
        keep = np.arange(self.n) != i
        m = xr.GPRRef(self.X[keep], self.Y[keep], self.kind, self.var, self.ls if self.ARD else self.ls[:1], self.noise, ARD=self.ARD,
                      mean=self.mean)
        mean, v = m.predict_y(self.X[i:i + 1])
        return mean[0], v[0, 0]


class LooTorch(xr.DirectGPR):
    """the fp64 statement: direct-difference K, torch.linalg.inv of Kyy, the sums above; gradients by autograd.  loss() = -L_LOO,
    so DirectGPR.loss_grads_with_mean and GPROracle.optimize_adam run on the leave-one-out objective."""

    def _pa(self):
        P = torch.linalg.inv(self.compute_kyy())
        return P, P @ (self.Y - self._mean(self.X))

    def loo(self):
        P, a = self._pa()
        p = P.diagonal()
        n, dy = a.shape
        return (0.5 * (dy * p.log() - (a * a).sum(1) / p)).sum() - 0.5 * n * dy * np.log(2 * np.pi)

    def loss(self):
        return -(self.loo() + 0.0).reshape(1)

    def loo_predict(self):
        with torch.no_grad():
            P, a = self._pa()
            p = P.diagonal()
            return self.Y - a / p[:, None], (1.0 / p)[:, None].expand_as(a)

    def G(self):
        with torch.no_grad():
            P, a = self._pa()
        return loo_G(P.numpy(), a.numpy(), np.float64)


def make_pair(x, y, kind, variance, length_scales, noise, ARD=False, mean=None):
    """(LooRef, LooTorch) of one model."""
    return (LooRef(x, y, kind, variance, length_scales, noise, ARD=ARD, mean=mean),
            LooTorch(x, y, kind=kind, variance=variance, length_scales=length_scales, noise=noise, ARD=ARD, mean=mean))
