"""
TEST INFRASTRUCTURE ONLY (never imported by the package) -- host statements of the FITC marginal likelihood
(Snelson & Ghahramani 2006) that share nothing with the streamed Woodbury evaluation of gptorch_amd/models/_fitc.py:

  - FITCOracle: the DENSE form in torch fp64 on the CPU.  Sigma = Q + diag(Kdiag - diag Q) + s2 I with Q = Kfu Kuu^-1 Kuf is
    built as an N x N matrix and factorised; log p(Y) = N(err | 0, Sigma) per output column, gradients by autograd w.r.t. the raw
    (log) parameters, Z and the mean, and the dense predictive equations  mean = Q*f Sigma^-1 err + m(x*),
    cov = K** - Q*f Sigma^-1 Qf*.
  - lml_ld / predict_ld: the same two in numpy long double (tests/_xref.py's Cholesky and solves).
  - closed_form_check: the closed-form backward of _fitc.py's docstring, restated in fp64 torch, against autograd through the
    dense form w.r.t. (Kuu, Kuf, Kdiag, s2, err).

Stationary kinds take their distances by direct differences (tests/_xref.py): Z is a subset of X in the golden cases.
"""
import math

import numpy as np
import torch

from oracle import gp_oracle as orc
from tests import _xref as xr

DTYPE = torch.float64
LD = xr.LD
COMPOSITE = "Linear+Rbf+Constant"


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64)).clone()


class FITCOracle:
    """kernel: dict(kind=<stationary kind>, variance, length_scales [, ARD]) or
    dict(kind="Linear+Rbf+Constant", linear_variance, variance, length_scales, constant)."""

    def __init__(self, x, y, z, kernel, noise, mean=None):
        self.X, self.Y = _t(x), _t(y)
        d = self.X.shape[1]
        self.kind = kernel["kind"]
        leaf = lambda v: torch.log(_t(np.atleast_1d(v))).requires_grad_(True)
        self.raw = {}
        if self.kind == COMPOSITE:
            self.raw["linear_variance"] = leaf(np.asarray(kernel["linear_variance"]) * np.ones(d))
            self.raw["constant"] = leaf(kernel["constant"])
        ls = kernel["length_scales"]
        if kernel.get("ARD"):
            ls = np.asarray(ls, dtype=np.float64) * np.ones(d)
        self.raw["variance"] = leaf(kernel["variance"])
        self.raw["length_scales"] = leaf(ls)
        self.raw["noise"] = leaf(noise)
        self.raw["Z"] = _t(z).requires_grad_(True)
        if mean is not None:
            self.raw["mean"] = _t(mean).requires_grad_(True)

    # ---- pieces (fp64, differentiable) ---------------------------------------------------------------------------------
    def K(self, a, b=None):
        var, ls = self.raw["variance"].exp(), self.raw["length_scales"].exp()
        if self.kind == COMPOSITE:
            rows, cols = a.shape[0], (a if b is None else b).shape[0]
            return orc.linear_K(a, b, self.raw["linear_variance"].exp()) + xr.direct_kernel_K("Rbf", a, b, var, ls) \
                + self.raw["constant"].exp().expand(rows, cols)
        return xr.direct_kernel_K(self.kind, a, b, var, ls)

    def Kdiag(self, a):
        var = self.raw["variance"].exp().expand(a.shape[0])
        if self.kind == COMPOSITE:
            return orc.linear_Kdiag(a, self.raw["linear_variance"].exp()) + var + self.raw["constant"].exp().expand(a.shape[0])
        return var

    def mean_at(self, a):
        if "mean" not in self.raw:
            return torch.zeros(a.shape[0], self.Y.shape[1], dtype=DTYPE)
        return self.raw["mean"].unsqueeze(0).expand(a.shape[0], -1)

    def err(self):
        return self.Y - self.mean_at(self.X)

    @staticmethod
    def dense_lml(Kuu, Kuf, Kdiag, s2, err):
        """log N(err | 0, Q + diag(Kdiag - diag Q) + s2 I) summed over the columns, through the N x N matrix."""
        n, p = err.shape
        A = orc.trtrs(Kuf, torch.linalg.cholesky(Kuu))
        Q = A.t() @ A
        Sigma = Q + torch.diag(Kdiag - Q.diagonal() + s2)
        Lc = torch.linalg.cholesky(Sigma)
        alpha = orc.trtrs(err, Lc)
        return -0.5 * p * n * math.log(2.0 * math.pi) - p * Lc.diagonal().log().sum() - 0.5 * alpha.pow(2).sum()

    @staticmethod
    def woodbury_lml(Kuu, Kuf, Kdiag, s2, err):
        """the same value through the M-sized (Woodbury) algebra: a second, algebraically different fp64 evaluation."""
        n, p = err.shape
        A = orc.trtrs(Kuf, torch.linalg.cholesky(Kuu))
        lam = Kdiag - A.pow(2).sum(0) + s2
        LB = torch.linalg.cholesky(torch.eye(Kuu.shape[0], dtype=DTYPE) + (A / lam) @ A.t())
        c = orc.trtrs((A / lam) @ err, LB)
        return -0.5 * p * n * math.log(2.0 * math.pi) - 0.5 * p * lam.log().sum() - p * LB.diagonal().log().sum() \
            - 0.5 * (err.pow(2) / lam[:, None]).sum() + 0.5 * c.pow(2).sum()

    def grad_e64(self):
        """No long-double gradient exists.  The distance between the autograd gradients of the two fp64 evaluations (dense and
        Woodbury), max |difference| / max(1, max |gradient|) over the parameter blocks, stands in for the fp64 error of a gradient."""
        out = 0.0
        names = list(self.raw)
        gd = torch.autograd.grad(-self.dense_lml(*self._inputs()), [self.raw[k] for k in names])
        gw = torch.autograd.grad(-self.woodbury_lml(*self._inputs()), [self.raw[k] for k in names])
        for a, b in zip(gd, gw):
            out = max(out, xr.rel_err(b, a))
        return out

    def _inputs(self):
        Z = self.raw["Z"]
        return self.K(Z), self.K(Z, self.X), self.Kdiag(self.X), self.raw["noise"].exp(), self.err()

    def log_likelihood(self):
        return self.dense_lml(*self._inputs()).reshape(())

    def loss(self):
        return -self.log_likelihood()

    def loss_and_grads(self):
        for q in self.raw.values():
            q.grad = None
        loss = self.loss()
        loss.backward()
        return loss.item(), {k: (q.grad.numpy().copy() if q.grad is not None else np.zeros(tuple(q.shape))) for k, q in self.raw.items()}

    def predict_f(self, x_new, diag=True):
        """dense predictive equations -> (mean [ns, dy], var [ns] or cov [ns, ns]) as numpy."""
        with torch.no_grad():
            xs = _t(x_new)
            Kuu, Kuf, Kd, s2, err = self._inputs()
            L = torch.linalg.cholesky(Kuu)
            A = orc.trtrs(Kuf, L)
            As = orc.trtrs(self.K(self.raw["Z"], xs), L)
            Q = A.t() @ A
            Lc = torch.linalg.cholesky(Q + torch.diag(Kd - Q.diagonal() + s2))
            V = orc.trtrs(A.t() @ As, Lc)                               # Lc^-1 Qf*
            mean = V.t() @ orc.trtrs(err, Lc) + self.mean_at(xs)
            if diag:
                return mean.numpy(), (self.Kdiag(xs) - V.pow(2).sum(0)).numpy()
            return mean.numpy(), (self.K(xs) - V.t() @ V).numpy()

    def predict_y(self, x_new, diag=True):
        mean, v = self.predict_f(x_new, diag)
        s2 = float(self.raw["noise"].exp())
        return mean, (v + s2 if diag else v + s2 * np.eye(v.shape[0]))

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

    # ---- long double ---------------------------------------------------------------------------------------------------
    def _K_ld(self, a, b=None):
        var, ls = xr.ld(self.raw["variance"].exp())[0], xr.ld(self.raw["length_scales"].exp())
        if self.kind == COMPOSITE:
            a_, b_ = xr.ld(a), xr.ld(a if b is None else b)
            return (a_ * xr.ld(self.raw["linear_variance"].exp())) @ b_.T + xr.K("Rbf", a, b, var, ls) + xr.ld(self.raw["constant"].exp())[0]
        return xr.K(self.kind, a, b, var, ls)

    def _Kdiag_ld(self, a):
        var = xr.ld(self.raw["variance"].exp())[0]
        if self.kind == COMPOSITE:
            a_ = xr.ld(a)
            return np.sum(a_ * a_ * xr.ld(self.raw["linear_variance"].exp()), 1) + var + xr.ld(self.raw["constant"].exp())[0]
        return xr.Kdiag(a, var)

    def _dense_ld(self):
        X, Z = self.X, self.raw["Z"].detach()
        s2 = xr.ld(self.raw["noise"].exp())[0]
        L = xr.cholesky(self._K_ld(Z))
        A = xr.solve_lower(L, self._K_ld(Z, X))
        Q = A.T @ A
        Lc = xr.cholesky(Q + np.diag(self._Kdiag_ld(X) - np.diag(Q) + s2))
        err = xr.ld(self.Y) - xr.ld(self.mean_at(self.X))
        return L, A, Lc, xr.solve_lower(Lc, err)

    def lml_ld(self):
        _, _, Lc, alpha = self._dense_ld()
        n, p = alpha.shape
        return -LD(0.5) * p * n * np.log(2 * LD(np.pi)) - p * np.sum(np.log(np.diag(Lc))) - LD(0.5) * np.sum(alpha ** 2)

    def predict_ld(self, x_new):
        """-> (mean [ns, dy], cov [ns, ns]) of the latent function in long double (the diagonal of cov is the variance)."""
        L, A, Lc, alpha = self._dense_ld()
        As = xr.solve_lower(L, self._K_ld(self.raw["Z"].detach(), x_new))
        V = xr.solve_lower(Lc, A.T @ As)
        return V.T @ alpha + xr.ld(self.mean_at(_t(x_new))), self._K_ld(x_new) - V.T @ V

    # ---- the closed-form backward of gptorch_amd/models/_fitc.py against autograd through the dense form -----------------------
    def closed_form_check(self):
        """max relative difference, over dF/d(Kuu, Kuf, Kdiag, s2, err), between the closed form and autograd."""
        with torch.no_grad():
            leaves = [t.detach().clone().requires_grad_(True) for t in self._inputs()]
        F = self.dense_lml(*leaves)
        auto = torch.autograd.grad(F, leaves)
        Kuu, Kuf, Kd, s2, err = [t.detach() for t in leaves]
        m, (n, p) = Kuu.shape[0], err.shape
        L = torch.linalg.cholesky(Kuu)
        A = orc.trtrs(Kuf, L)
        lam = Kd - A.pow(2).sum(0) + s2
        B = torch.eye(m, dtype=DTYPE) + (A / lam) @ A.t()
        Binv = torch.linalg.inv(B)
        beta = Binv @ ((A / lam) @ err)
        r = (err - A.t() @ beta) / lam[:, None]
        g = r.pow(2).sum(1) - p * (1.0 / lam - ((Binv @ A) * A).sum(0) / lam ** 2)
        dA = beta @ r.t() - p * (Binv @ A) / lam - A * g
        U = torch.linalg.inv(L).t()
        S = beta @ beta.t() - p * (torch.eye(m, dtype=DTYPE) - Binv) - (A * g) @ A.t()
        closed = [-0.5 * U @ S @ U.t(), U @ dA, 0.5 * g, (0.5 * g.sum()).reshape(s2.shape), -r]
        auto = [0.5 * (auto[0] + auto[0].t())] + list(auto[1:])
        return max(float((c - a).abs().max() / max(1.0, float(a.abs().max()))) for c, a in zip(closed, auto))


# ---- the golden cases (tests/golden/fitc_cases.json): inputs regenerated from their seeds -----------------------------------
def case_inputs(case):
    """-> dict(x, y, z, xs): Z is a subset of X (every n // m-th row), xs 16 test points."""
    from gptorch_amd import rng
    n, d, dy, m = case["n"], case["d"], case["dy"], case["m"]
    x, y = rng.make_regression(n, d, dy, seed=case["seed_x"])
    return dict(x=x, y=y, z=x[:: n // m][:m].copy(), xs=rng.normal(case["seed_xs"], (16, d)))


def oracle_for(case, inp):
    return FITCOracle(inp["x"], inp["y"], inp["z"], case["kernel"], case["noise"], mean=case.get("mean"))


def model_names(case):
    """oracle parameter name -> parameter name of the model."""
    names = {"Z": "Z", "noise": "likelihood.variance"}
    if case["kernel"]["kind"] == COMPOSITE:
        names.update({"linear_variance": "kernel.kern1.kern1.variance", "variance": "kernel.kern1.kern2.variance",
                      "length_scales": "kernel.kern1.kern2.length_scales", "constant": "kernel.kern2.variance"})
    else:
        names.update({"variance": "kernel.variance", "length_scales": "kernel.length_scales"})
    if case.get("mean") is not None:
        names["mean"] = "mean_function.val"
    return names


def build_kernel(kernels, case):
    k, d = case["kernel"], case["d"]
    if k["kind"] == COMPOSITE:
        return kernels.Linear(d, variance=k["linear_variance"]) + kernels.Rbf(d, variance=k["variance"], length_scales=k["length_scales"]) \
            + kernels.Constant(d, variance=k["constant"])
    ls = k["length_scales"]
    if k.get("ARD"):
        ls = np.asarray(ls, dtype=np.float64) * np.ones(d)
    return getattr(kernels, k["kind"])(d, variance=k["variance"], length_scales=ls, ARD=bool(k.get("ARD")))


def build_model(case, inp, cls=None):
    """the case's model from gptorch_amd (cls: FITC by default; VFE / GPR for the property tests)."""
    import gptorch_amd
    from gptorch_amd import kernels, likelihoods, mean_functions
    cls = gptorch_amd.models.FITC if cls is None else cls
    mean = None
    if case.get("mean") is not None:
        mean = mean_functions.Constant(case["dy"], val=torch.tensor(case["mean"], dtype=DTYPE))
    return cls(inp["x"], inp["y"], build_kernel(kernels, case), inducing_points=inp["z"].copy(), mean_function=mean,
               likelihood=likelihoods.Gaussian(variance=case["noise"]))
