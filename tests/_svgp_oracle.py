"""
Host statement of the SVGP bound (Hensman et al. 2013), plain fp64 torch on the CPU: marginals of q(f), KL(q(u) || p(u)),
the minibatch-scaled bound, prediction, and gradients by autograd.  Test infrastructure only (never imported by the
package): tests/golden/make_svgp_golden.py asserts that it agrees with the reference (gptorch/models/sparse_gpr.py:198-381)
on every case it writes, and the GPU tests hold the native path against it on shapes no golden covers.

Parameters live in the RAW space the optimisers see: log of every positive value, and for the Cholesky factor S_L of q(u)'s
covariance the strictly-lower entries as they are with the LOG of the diagonal (torch's LowerCholeskyTransform).
"""
import math

import numpy as np
import torch

from oracle import gp_oracle as orc

DTYPE = torch.float64


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64)).clone()


def chol_to_raw(S_L):
    S_L = _t(S_L)
    return S_L.tril(-1) + S_L.diagonal().log().diag()


def raw_to_chol(raw):
    return raw.tril(-1) + raw.diagonal().exp().diag()


class SVGPOracle:
    """kernel: dict(kind=<stationary kind>, variance, length_scales [, ARD]) or
    dict(kind="Linear+Rbf+Constant", linear_variance, variance, length_scales, constant) -- the reference's example model."""

    def __init__(self, x, y, z, kernel, noise=1.0, q_mu=None, q_sqrt=None, mean=None, batch_size=None):
        self.X, self.Y = _t(x), _t(y)
        self.batch_size = batch_size
        d = self.X.shape[1]
        self.kind = kernel["kind"]
        leaf = lambda v: torch.log(_t(np.atleast_1d(v))).requires_grad_(True)
        self.raw = {}
        if self.kind == "Linear+Rbf+Constant":
            self.raw["linear_variance"] = leaf(np.asarray(kernel["linear_variance"]) * np.ones(d))
            self.raw["constant"] = leaf(kernel["constant"])
        ls = kernel["length_scales"]
        if kernel.get("ARD"):
            ls = np.asarray(ls, dtype=np.float64) * np.ones(d)
        self.raw["variance"] = leaf(kernel["variance"])
        self.raw["length_scales"] = leaf(ls)
        self.raw["noise"] = leaf(noise)
        self.raw["Z"] = _t(z).requires_grad_(True)
        m, dy = self.raw["Z"].shape[0], self.Y.shape[1]
        self.raw["q_mu"] = (_t(q_mu) if q_mu is not None else torch.zeros(m, dy, dtype=DTYPE)).requires_grad_(True)
        self.raw["q_sqrt"] = chol_to_raw(q_sqrt if q_sqrt is not None else np.eye(m)).requires_grad_(True)
        self.mean = None
        if mean is not None:
            self.raw["mean"] = _t(mean).requires_grad_(True)

    # ---- pieces -----------------------------------------------------------------------------------------------------
    def K(self, a, b=None):
        var, ls = self.raw["variance"].exp(), self.raw["length_scales"].exp()
        if self.kind == "Linear+Rbf+Constant":
            rows, cols = a.shape[0], (a if b is None else b).shape[0]
            return orc.linear_K(a, b, self.raw["linear_variance"].exp()) + orc.kernel_K("Rbf", a, b, var, ls) \
                + self.raw["constant"].exp().expand(rows, cols)
        return orc.kernel_K(self.kind, a, b, var, ls)

    def Kdiag(self, a):
        var = self.raw["variance"].exp().expand(a.shape[0])
        if self.kind == "Linear+Rbf+Constant":
            return orc.linear_Kdiag(a, self.raw["linear_variance"].exp()) + var + self.raw["constant"].exp().expand(a.shape[0])
        return var

    def mean_at(self, a):
        if "mean" not in self.raw:
            return torch.zeros(a.shape[0], self.Y.shape[1], dtype=DTYPE)
        return self.raw["mean"].unsqueeze(0).expand(a.shape[0], -1)

    def _factors(self):
        L = orc.cholesky(self.K(self.raw["Z"]))
        S_L = raw_to_chol(self.raw["q_sqrt"])
        return L, S_L

    def marginals(self, a, full=False):
        """q(f) at the rows of `a`: (mean [n, dy], variance [n] or covariance [n, n])."""
        L, S_L = self._factors()
        Z = self.raw["Z"]
        alpha = orc.trtrs(self.K(Z, a), L).t()                     # K(a, Z) L^-T
        beta = orc.trtrs(S_L, L)                                   # L^-1 S_L
        mean = alpha @ orc.trtrs(self.raw["q_mu"], L) + self.mean_at(a)
        gamma = alpha @ beta
        if full:
            return mean, self.K(a) - alpha @ alpha.t() + gamma @ gamma.t()
        return mean, self.Kdiag(a) - alpha.pow(2).sum(1) + gamma.pow(2).sum(1)

    def kl(self):
        """sum over output columns of KL(N(q_mu_j + m(Z), S) || N(m(Z), K(Z))): the prior mean cancels."""
        L, S_L = self._factors()
        m, dy = self.raw["q_mu"].shape
        beta = orc.trtrs(S_L, L)
        w = orc.trtrs(self.raw["q_mu"], L)
        return 0.5 * dy * (beta.pow(2).sum() - m + 2.0 * L.diagonal().log().sum() - 2.0 * S_L.diagonal().log().sum()) \
            + 0.5 * w.pow(2).sum()

    def expected_log_lik(self, mean, var, y):
        """E_q[log N(y | f, noise)] summed over rows and output columns (the same variance for every column)."""
        s2 = self.raw["noise"].exp()
        n, dy = y.shape
        return (-0.5 * (n * dy * (math.log(2.0 * math.pi) + torch.log(s2)) + ((y - mean).pow(2).sum() + dy * var.sum()) / s2)).reshape(())

    # ---- the bound --------------------------------------------------------------------------------------------------
    def draw(self):
        """the minibatch rule: one host permutation per evaluation when batch_size is set."""
        if self.batch_size is None:
            return self.X, self.Y
        i = np.random.permutation(self.X.shape[0])[: self.batch_size]
        return self.X[i, :], self.Y[i, :]

    def log_likelihood(self, x=None, y=None, idx=None):
        if idx is not None:
            x, y = self.X[idx], self.Y[idx]
        elif x is None:
            x, y = self.draw()
        else:
            x, y = _t(x), _t(y)
        mean, var = self.marginals(x)
        return self.expected_log_lik(mean, var, y) * (self.X.shape[0] / x.shape[0]) - self.kl()

    def loss(self, **kw):
        return -self.log_likelihood(**kw)

    def loss_and_grads(self, **kw):
        for p in self.raw.values():
            p.grad = None
        loss = self.loss(**kw)
        loss.backward()
        return loss.item(), {k: (p.grad.numpy().copy() if p.grad is not None else np.zeros(tuple(p.shape))) for k, p in self.raw.items()}

    def predict_f(self, x_new, diag=True):
        with torch.no_grad():
            mean, v = self.marginals(_t(x_new), full=not diag)
        return mean.numpy(), v.numpy()

    def optimize_adam(self, steps, learning_rate=0.01):
        opt = torch.optim.Adam(list(self.raw.values()), lr=learning_rate)
        losses = []
        for _ in range(steps):
            opt.zero_grad()
            loss = self.loss()
            loss.backward()
            opt.step()
            losses.append(loss.item())
        return losses


# ---- inputs of the golden cases (tests/golden/svgp_cases.json), regenerated from their seeds ------------------------------
def case_inputs(case, z=None):
    """-> dict(x, y, z, q_mu, q_sqrt, xs, idx): everything a case needs that is not stored with it."""
    from gptorch_amd import rng
    n, d, dy, m = case["n"], case["d"], case["dy"], case["m"]
    x, y = rng.make_regression(n, d, dy, seed=case["seed_x"])
    if z is None:
        z = x[:: n // m][:m] + 0.05 * rng.normal(case["seed_z"], (m, d))      # spread like the data, no coincident points
    q_mu = 0.5 * rng.normal(case["seed_q"], (m, dy))
    A = rng.normal(case["seed_q"] + 1, (m, m))
    q_sqrt = np.tril(A, -1) * (0.3 / np.sqrt(m)) + np.diag(0.4 + 0.2 * np.abs(np.diag(A)))
    xs = rng.normal(case["seed_xs"], (16, d))
    idx = None
    if case.get("nb") is not None:
        idx = np.random.RandomState(case["seed_idx"]).permutation(n)[: case["nb"]]
    return dict(x=x, y=y, z=z, q_mu=q_mu, q_sqrt=q_sqrt, xs=xs, idx=idx)


def oracle_for(case, inp, batch_size=None):
    return SVGPOracle(inp["x"], inp["y"], inp["z"], case["kernel"], noise=case["noise"], q_mu=inp["q_mu"], q_sqrt=inp["q_sqrt"],
                      mean=case.get("mean"), batch_size=batch_size)


# oracle parameter name -> parameter name of the models (ours and the reference's share them)
def model_names(case):
    names = {"Z": "Z", "q_mu": "induced_output_mean", "q_sqrt": "induced_output_chol_cov", "noise": "likelihood.variance"}
    if case["kernel"]["kind"] == "Linear+Rbf+Constant":
        names.update({"linear_variance": "kernel.kern1.kern1.variance", "variance": "kernel.kern1.kern2.variance",
                      "length_scales": "kernel.kern1.kern2.length_scales", "constant": "kernel.kern2.variance"})
    else:
        names.update({"variance": "kernel.variance", "length_scales": "kernel.length_scales"})
    if case.get("mean") is not None:
        names["mean"] = "mean_function.val"
    return names


def build_model(pkg, case, inp, batch_size=None):
    """the same model from package `pkg` (gptorch_amd, or the reference in the generator), parameters set to the case's."""
    k, d = case["kernel"], case["d"]
    if k["kind"] == "Linear+Rbf+Constant":
        kern = pkg.kernels.Linear(d, variance=k["linear_variance"]) + pkg.kernels.Rbf(d, variance=k["variance"], length_scales=k["length_scales"]) \
            + pkg.kernels.Constant(d, variance=k["constant"])
    else:
        ls = k["length_scales"]
        if k.get("ARD"):
            ls = np.asarray(ls, dtype=np.float64) * np.ones(d)
        kern = getattr(pkg.kernels, k["kind"])(d, variance=k["variance"], length_scales=ls, ARD=bool(k.get("ARD")))
    mean = None
    if case.get("mean") is not None:
        mean = pkg.mean_functions.Constant(case["dy"], val=torch.tensor(case["mean"], dtype=DTYPE))
    np.random.seed(0)                                                         # (the constructor's own draw; overwritten below)
    model = pkg.models.SVGP(inp["x"], inp["y"], kern, inducing_points=inp["z"].copy(), mean_function=mean,
                            likelihood=pkg.likelihoods.Gaussian(variance=case["noise"]), batch_size=batch_size)
    model.induced_output_mean.data = _t(inp["q_mu"])
    model.induced_output_chol_cov.data = chol_to_raw(inp["q_sqrt"])
    return model
