"""
TEST INFRASTRUCTURE ONLY -- k-fold cross-validation of the exact GP in closed form from the diagonal blocks of the inverse, stated
twice on the host: in numpy's long double on top of tests/_xref.GPRRef (KFoldRef), and in plain fp64 (KFoldTorch: torch, a dense
LAPACK inverse, gradients by autograd; kfold_terms with dtype=np.float64: the same sums in numpy fp64).  With P = Kyy^-1,
r = Y - m, a = P r, a fold with index set I of m_f points and P_f = P[I, I]:

    y_I - mu_I = q_I = P_f^-1 a_I            Sigma_f = P_f^-1            (the predictive of the OBSERVATIONS y_I given every other fold)
    log p(y_I | y_-I) = -1/2 sum_c a_Ic^T q_Ic + 1/2 dy log|P_f| - 1/2 m_f dy log 2 pi,   L_kfold = sum_f log p(y_I | y_-I)
    D = blockdiag_f 1/2 (dy Sigma_f + q_I q_I^T),  w = P q,  Q = P D P
    dL_kfold/dtheta = sum_ij G_ij dKyy_ij/dtheta,  G = -Q + 1/2 (a w^T + w a^T),  dL/dnoise = tr G,  dL/dr = -w

(the leave-one-out closed form of tests/_loo_oracle.py with diag(d) replaced by a block diagonal D; every m_f = 1 gives it back).
KFoldRef.refit(f) does NOT use any of this: it deletes the fold's rows, factorises the rest, predicts y_I with its full covariance
and evaluates the multivariate normal log density.

gptorch_amd never imports this module.
"""
import numpy as np
import torch

from tests import _xref as xr

LD = xr.LD
U = 2.0 ** -53


def partition(folds, n):
    """the folds as a list of int64 index arrays: an int k means np.array_split(np.arange(n), k)"""
    if isinstance(folds, (int, np.integer)):
        return [np.asarray(p, dtype=np.int64) for p in np.array_split(np.arange(n), int(folds))]
    return [np.asarray(p, dtype=np.int64) for p in folds]


def _inverse_spd(A, dtype):
    """(A^-1, log|A|) of a small SPD matrix in `dtype` (long double: tests/_xref's Cholesky; fp64: LAPACK's)"""
    m = A.shape[0]
    if dtype is LD:
        L = xr.cholesky(A)
        Li = xr.solve_lower(L, np.eye(m, dtype=LD))
        return np.einsum("ki,kj->ij", Li, Li), 2 * np.sum(np.log(np.diag(L)))
    L = np.linalg.cholesky(A)
    Li = np.linalg.solve(L, np.eye(m))
    return Li.T @ Li, 2 * np.sum(np.log(np.diag(L)))


def kfold_terms(P, a, parts, dtype=LD):
    """from the full symmetric P [n, n], a = P r [n, dy] and the folds: (q [n, dy] and var [n] in data order, the blocks
    D_f = 1/2 (dy Sigma_f + q_I q_I^T), logdet [k] = log|P_f|, quad [k] = sum_c a_Ic^T q_Ic, value = L_kfold) in `dtype`."""
    P, a = np.asarray(P, dtype=dtype), np.asarray(a, dtype=dtype)
    n, dy = a.shape
    q, var = np.zeros((n, dy), dtype=dtype), np.zeros(n, dtype=dtype)
    blocks, logdet, quad = [], np.zeros(len(parts), dtype=dtype), np.zeros(len(parts), dtype=dtype)
    for f, I in enumerate(parts):
        Sigma, logdet[f] = _inverse_spd(P[np.ix_(I, I)], dtype)
        q[I] = Sigma @ a[I]
        var[I] = np.diag(Sigma)
        quad[f] = np.sum(a[I] * q[I])
        blocks.append(dtype(0.5) * (dy * Sigma + q[I] @ q[I].T))
    value = np.sum(dtype(0.5) * (dy * logdet - quad)) - dtype(0.5) * n * dy * np.log(2 * dtype(np.pi))
    return q, var, blocks, logdet, quad, value


def kfold_G(P, a, parts, dtype=LD):
    """(G [n, n], w [n, dy]) from the full symmetric P and a."""
    P, a = np.asarray(P, dtype=dtype), np.asarray(a, dtype=dtype)
    q, _, blocks, _, _, _ = kfold_terms(P, a, parts, dtype)
    w = P @ q
    Q = np.zeros_like(P)
    for I, D in zip(parts, blocks):
        Q += P[:, I] @ D @ P[I, :]
    return -Q + dtype(0.5) * (a @ w.T + w @ a.T), w


class KFoldRef(xr.GPRRef):
    """GPRRef plus the k-fold closed form, every intermediate in long double."""

    def __init__(self, x, y, kind, variance=None, length_scales=None, noise=None, ARD=False, mean=None, folds=None):
        super().__init__(x, y, kind, variance, length_scales, noise, ARD=ARD, mean=mean)
        self.parts = partition(folds, self.n)
        Li = xr.solve_lower(self.L, np.eye(self.n, dtype=LD))
        self.P = np.einsum("ki,kj->ij", Li, Li)
        self.a = xr.solve_upper_t(self.L, self.alpha)
        self.q, self.s2, self.blocks, self.logdet, self.quad, self.value = kfold_terms(self.P, self.a, self.parts)

    def kfold(self):
        return self.value

    def loss(self):
        return -self.value

    def fold_log_density(self, f):
        """log p(y_I | y_-I) of fold f, in closed form"""
        return LD(0.5) * (self.dy * self.logdet[f] - self.quad[f]) - LD(0.5) * self.parts[f].size * self.dy * np.log(2 * LD(np.pi))

    def kfold_predict(self):
        return self.Y - self.q, np.repeat(self.s2[:, None], self.dy, 1)

    def G(self):
        return kfold_G(self.P, self.a, self.parts)

    def loss_grads(self):
        """d(-L_kfold) / d(log variance, log ell [d or 1], log noise, mean [dy]), as GPRRef.loss_grads orders them."""
        G, w = self.G()
        g_var, g_ls = xr.kernel_param_grads(self.kind, self.X, None, self.var, self.ls, G, self.ARD)
        return [-g_var, -g_ls, -np.array([self.noise * np.trace(G)]), -w.sum(0)]

    def refit(self, f):
        """(log p(y_I | y_-I), mean [m_f, dy], variances [m_f]) of fold f from a model that never saw it: a fresh GPRRef on the other
        rows, its predictive of the observations with the full covariance, the multivariate normal log density in long double."""
        I = self.parts[f]
        keep = np.ones(self.n, dtype=bool)
        keep[I] = False
        m = xr.GPRRef(self.X[keep], self.Y[keep], self.kind, self.var, self.ls if self.ARD else self.ls[:1], self.noise, ARD=self.ARD,
                      mean=self.mean)
        mean, cov = m.predict_y(self.X[I], diag=False)
        Lc = xr.cholesky(cov)
        z = xr.solve_lower(Lc, self.Y[I] - mean)
        logp = -LD(0.5) * np.sum(z * z) - self.dy * np.sum(np.log(np.diag(Lc))) - LD(0.5) * I.size * self.dy * np.log(2 * LD(np.pi))
        return logp, mean, np.diag(cov)


class KFoldTorch(xr.DirectGPR):
    """the fp64 statement: direct-difference K, torch.linalg.inv of Kyy, the sums above fold by fold; gradients by autograd.
    loss() = -L_kfold, so DirectGPR.loss_grads_with_mean and GPROracle.optimize_adam run on the k-fold objective."""

    def __init__(self, x, y, kind="Rbf", variance=1.0, length_scales=1.0, noise=None, ARD=False, mean=None, folds=None):
        super().__init__(x, y, kind=kind, variance=variance, length_scales=length_scales, noise=noise, ARD=ARD, mean=mean)
        self.parts = [torch.as_tensor(p) for p in partition(folds, self.X.shape[0])]

    def _pa(self):
        P = torch.linalg.inv(self.compute_kyy())
        return P, P @ (self.Y - self._mean(self.X))

    def kfold(self):
        P, a = self._pa()
        n, dy = a.shape
        total = -0.5 * n * dy * np.log(2 * np.pi)
        for I in self.parts:
            Pf, aI = P[I][:, I], a[I]
            total = total + 0.5 * dy * torch.linalg.slogdet(Pf)[1] - 0.5 * (aI * torch.linalg.solve(Pf, aI)).sum()
        return total

    def loss(self):
        return -(self.kfold() + 0.0).reshape(1)

    def kfold_predict(self):
        with torch.no_grad():
            P, a = self._pa()
            mean, var = torch.empty_like(a), torch.empty_like(a)
            for I in self.parts:
                Sigma = torch.linalg.inv(P[I][:, I])
                mean[I] = self.Y[I] - Sigma @ a[I]
                var[I] = Sigma.diagonal()[:, None].expand(I.numel(), a.shape[1])
            return mean, var


def make_pair(x, y, kind, variance, length_scales, noise, ARD=False, mean=None, folds=None):
    """(KFoldRef, KFoldTorch) of one model."""
    return (KFoldRef(x, y, kind, variance, length_scales, noise, ARD=ARD, mean=mean, folds=folds),
            KFoldTorch(x, y, kind=kind, variance=variance, length_scales=length_scales, noise=noise, ARD=ARD, mean=mean, folds=folds))
