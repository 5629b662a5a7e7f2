"""Likelihoods: the Gaussian of gptorch/likelihoods.py:80-144 (the only one on the GPR path) and, for SVGP, the Gauss-Hermite
quadrature that the reference's Likelihood names and leaves as a TODO (likelihoods.py:47-78), with Bernoulli, Poisson and
Student-t likelihoods on top of it.

The quadrature rule, for q(f) = N(mu, v) and the physicists' nodes x_h and weights w_h of numpy's hermgauss(H):

    E_q[g(f)]  ~=  pi^-1/2 sum_h w_h g(mu + sqrt(2 v) x_h)

Everything in this file is plain torch (CPU or GPU, differentiable by autograd).  On the GPU, SVGP evaluates the data term of
the four new classes with ONE fused kernel instead (csrc/lik.hip through models/sparse_gpr.py, NATIVE_EXPECTATION): the same
rule and its exact derivatives.  Bernoulli and Poisson also state logp_derivatives (logp and its first three derivatives in f):
what models.LaplaceGP's Newton search needs, evaluated on the GPU by csrc/laplace.hip with the same closed forms.

MultiClass (the robust-max likelihood over num_classes latent functions) COUPLES the latent columns of a row: it declares
num_latent, SVGP then carries that many columns over one column of labels, and its expectation and predictive probabilities are
variational_expectation / predict_mean_variance over all columns of a row at once -- plain torch here as well, and on the GPU one
fused launch each (csrc/multiclass.hip, under the same NATIVE_EXPECTATION switch).
"""
import math

import numpy as np
import torch

from .model import Model
from .param import Param
from .settings import DefaultPositiveTransform
from .util import torch_dtype

MAX_GAUSS_HERMITE_POINTS = 64   # what the fused kernel stages in LDS (csrc/lik.hip)
_GH_CACHE = {}


def gauss_hermite(H, device=None):
    """-> (nodes [H], weights [H]) of numpy.polynomial.hermite.hermgauss(H) as fp64 tensors on `device`, cached per (H, device)."""
    device = torch.device("cpu") if device is None else torch.device(device)
    key = (int(H), str(device))
    if key not in _GH_CACHE:
        x, w = np.polynomial.hermite.hermgauss(int(H))
        _GH_CACHE[key] = (torch.tensor(x, dtype=torch_dtype, device=device), torch.tensor(w, dtype=torch_dtype, device=device))
    return _GH_CACHE[key]


def _check_gaussian(qf, targets):
    """the checks of Gaussian.propagate_log (likelihoods.py:126-136) -> (mu, v)."""
    if not isinstance(qf, (torch.distributions.Normal, torch.distributions.MultivariateNormal)):
        raise TypeError("Expect Gaussian q(f)")
    mu, v = qf.loc, qf.variance
    n = targets.nelement()
    if not mu.nelement() == n:
        raise ValueError("Targets (%i) and q(f) (%i) have mismatch in size" % (n, mu.nelement()))
    return mu, v


class Likelihood(Model):
    """x -(GP)-> f -(likelihood)-> y.  A subclass that defines logp(F, Y) inherits propagate_log; one that defines
    conditional_mean(F) and conditional_variance(F) inherits predict_mean_variance; both by Gauss-Hermite quadrature with
    num_gauss_hermite_points nodes."""

    def __init__(self):
        super().__init__()
        self._num_gauss_hermite_points = 20

    @property
    def num_gauss_hermite_points(self):
        return self._num_gauss_hermite_points

    @num_gauss_hermite_points.setter
    def num_gauss_hermite_points(self, H):
        if not (isinstance(H, (int, np.integer)) and 1 <= H <= MAX_GAUSS_HERMITE_POINTS):
            raise ValueError("num_gauss_hermite_points must be an integer in [1, %d]; got %r" % (MAX_GAUSS_HERMITE_POINTS, H))
        self._num_gauss_hermite_points = int(H)

    def forward(self):
        return None

    def _quadrature(self, mu, v):
        """-> (f [..., H] = mu + sqrt(2 v) x_h, pi^-1/2 w [H])."""
        x, w = gauss_hermite(self.num_gauss_hermite_points, mu.device)
        return mu.unsqueeze(-1) + torch.sqrt(2.0 * v).unsqueeze(-1) * x, w * (1.0 / math.sqrt(math.pi))

    def propagate_log(self, qf, targets):
        """<log p(y|f)>_q(f) summed over the entries (likelihoods.py:70-78: "Implement quadrature fallback")."""
        mu, v = _check_gaussian(qf, targets)
        f, w = self._quadrature(mu, v)
        return (self.logp(f, targets.reshape(mu.shape).unsqueeze(-1)) * w).sum(-1).sum()

    def predict_mean_variance(self, mean_f, var_f):
        """mean and variance of y under p(y) = int p(y|f) N(f; mean_f, var_f) df (likelihoods.py:47-64: "TODO: Gauss-Hermite
        quadrature"): E[y] = <m(f)>, Var[y] = <s(f) + m(f)^2> - E[y]^2 with the conditional mean m and variance s."""
        f, w = self._quadrature(mean_f, var_f.expand_as(mean_f))
        m = self.conditional_mean(f)
        mean = (m * w).sum(-1)
        return mean, ((self.conditional_variance(f) + m * m) * w).sum(-1) - mean * mean

    def logp(self, F, Y):
        raise NotImplementedError("%s defines no logp(F, Y)" % type(self).__name__)

    def logp_derivatives(self, F, Y):
        """-> (logp, d1 = dlogp/dF, W = -d2logp/dF2, d3 = d3logp/dF3) in closed form: what a Newton search for the posterior
        mode needs (models.LaplaceGP)."""
        raise NotImplementedError("%s defines no logp_derivatives(F, Y)" % type(self).__name__)

    def conditional_mean(self, F):
        raise NotImplementedError("%s defines no conditional_mean(F)" % type(self).__name__)

    def conditional_variance(self, F):
        raise NotImplementedError("%s defines no conditional_variance(F)" % type(self).__name__)


class Gaussian(Likelihood):
    """(Spherical) Gaussian likelihood p(y|f) with variance Param (likelihoods.py:86-90)."""

    def __init__(self, variance=1.0):
        super().__init__()
        self.variance = Param(torch.tensor([float(variance)], dtype=torch_dtype),
                              transform=DefaultPositiveTransform())

    def logp(self, F, Y):
        """likelihoods.py:92-104."""
        return torch.distributions.Normal(F, torch.sqrt(self.variance.transform())).log_prob(Y)

    def predict_mean_variance(self, mean_f, var_f):
        """likelihoods.py:106-120."""
        return mean_f, var_f + self.variance.transform().expand_as(var_f)

    def predict_mean_covariance(self, mean_f, cov_f):
        """likelihoods.py:122-123."""
        return mean_f, cov_f + self.variance.transform().expand_as(cov_f).diag().diag()

    def propagate_log(self, qf, targets):
        """likelihoods.py:125-144."""
        if not isinstance(qf, (torch.distributions.Normal, torch.distributions.MultivariateNormal)):
            raise TypeError("Expect Gaussian q(f)")
        mu, s = qf.loc, qf.variance
        n = targets.nelement()
        if not mu.nelement() == n:
            raise ValueError("Targets (%i) and q(f) (%i) have mismatch in size" % (n, mu.nelement()))
        sigma_y = self.variance.transform()
        return -0.5 * (n * (math.log(2.0 * math.pi) + torch.log(sigma_y))
                       + (torch.sum((targets - mu) ** 2) + s.sum()) / sigma_y)


class _NonGaussian(Likelihood):
    """what the non-Gaussian likelihoods share: p(y) is no Gaussian, so nothing may add a noise covariance and sample one."""

    def predict_mean_covariance(self, mean_f, cov_f):
        raise NotImplementedError("%s has no Gaussian predictive distribution: use predict_y(diag=True) for its mean and variance"
                                  % type(self).__name__)


class _LogNdtr(torch.autograd.Function):
    """log Phi(z) (torch.special.log_ndtr) with the tail-stable derivative phi / Phi = sqrt(2 / pi) / erfcx(-z / sqrt 2) for
    z < 0: log_ndtr's own backward forms exp(-z^2 / 2 - log Phi(z)), the difference of two numbers of size z^2 / 2."""

    @staticmethod
    def forward(ctx, z):
        ctx.save_for_backward(z)
        return torch.special.log_ndtr(z)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        z, = ctx.saved_tensors
        neg = math.sqrt(2.0 / math.pi) / torch.special.erfcx(-z * math.sqrt(0.5))
        pos = torch.exp(-0.5 * z * z) * (1.0 / math.sqrt(2.0 * math.pi)) / (1.0 - 0.5 * torch.erfc(z * math.sqrt(0.5)))
        return g * torch.where(z < 0.0, neg, pos)


class Bernoulli(_NonGaussian):
    """y in {0, 1} with p(y = 1 | f) = Phi(f) (link="probit") or sigma(f) (link="logit").  With s = 2y - 1: logp = log Phi(s f)
    (probit) or -softplus(-s f) (logit).  Predictive mean and variance: CLOSED FORM for the probit link, p = Phi(mu / sqrt(1 + v))
    and p (1 - p); by quadrature for the logit link."""

    def __init__(self, link="probit"):
        super().__init__()
        if link not in ("probit", "logit"):
            raise ValueError("link must be 'probit' or 'logit'; got %r" % (link,))
        self.link = link

    def logp(self, F, Y):
        z = (2.0 * Y - 1.0) * F
        if self.link == "probit":
            return _LogNdtr.apply(z)
        return torch.nn.functional.logsigmoid(z)             # = -softplus(-z), without softplus's linear threshold

    def logp_derivatives(self, F, Y):
        """the closed forms of csrc/laplace.hip.  Probit, with t = 2y - 1, z = t f and the hazard r = phi(z) / Phi(z) (erfcx for
        z < 0): d1 = t r, W = r (z + r), d3 = t r ((z + r)(z + 2 r) - 1).  Logit, with e = exp(-|f|): d1 = t sigma(-z),
        W = e / (1 + e)^2, d3 = W tanh(f / 2) = W sign(f) (1 - e) / (1 + e) -- nothing overflows."""
        t = 2.0 * Y - 1.0
        z = t * F
        if self.link == "probit":
            zn, zp = torch.clamp(z, max=0.0), torch.clamp(z, min=0.0)          # each branch on its own side only
            neg = math.sqrt(2.0 / math.pi) / torch.special.erfcx(-zn * math.sqrt(0.5))
            pos = torch.exp(-0.5 * zp * zp) * (1.0 / math.sqrt(2.0 * math.pi)) / (1.0 - 0.5 * torch.erfc(zp * math.sqrt(0.5)))
            r = torch.where(z < 0.0, neg, pos)
            zr = z + r
            return torch.special.log_ndtr(z), t * r, r * zr, t * r * (zr * (zr + r) - 1.0)
        e = torch.exp(-torch.abs(F))
        q = 1.0 + e
        W = e / (q * q)
        return (torch.nn.functional.logsigmoid(z), t * (torch.where(z >= 0.0, e, torch.ones_like(e)) / q), W,
                W * (torch.sign(F) * -torch.expm1(-torch.abs(F)) / q))

    def conditional_mean(self, F):
        return torch.special.ndtr(F) if self.link == "probit" else torch.sigmoid(F)

    def conditional_variance(self, F):
        p = self.conditional_mean(F)
        return p * (1.0 - p)

    def predict_mean_variance(self, mean_f, var_f):
        if self.link == "probit":
            p = torch.special.ndtr(mean_f / torch.sqrt(1.0 + var_f))
        else:
            # a Bernoulli variable: Var[y] = E[y] (1 - E[y]) whatever the link; E[y] by the rule
            f, w = self._quadrature(mean_f, var_f.expand_as(mean_f))
            p = (torch.sigmoid(f) * w).sum(-1)
        return p, p * (1.0 - p)


class MultiClass(_NonGaussian):
    """y in {0, ..., C - 1} with the robust-max likelihood (Hernandez-Lobato et al. 2011) over C = num_classes latent functions:
    p(y | f) = 1 - epsilon if y = argmax_c f_c, else epsilon / (C - 1).  The likelihood COUPLES the latent columns of a row, so
    a model asks for `num_latent` columns and calls variational_expectation / predict_mean_variance with all of them; the
    per-column propagate_log does not apply.  Under q(f_c) = N(mu_c, v) with ONE variance per row (SVGP's marginals: S_L is
    shared by the columns) and the rule's nodes x_h and weights w_h:

        P = pi^-1/2 sum_h w_h prod_{c != y} Phi((mu_y - mu_c) / sqrt(v) + sqrt(2) x_h)      (the labelled latent is the largest)
        <log p(y | f)> = P log(1 - epsilon) + (1 - P) log(epsilon / (C - 1))

    -- linear in P, so nothing is ill-conditioned where P is tiny; far on the wrong side P and its gradients are exactly 0.  On
    the GPU an instance of exactly this type evaluates both methods with one fused launch each (csrc/multiclass.hip)."""

    def __init__(self, num_classes, epsilon=1e-3):
        super().__init__()
        if not (isinstance(num_classes, (int, np.integer)) and num_classes >= 2):
            raise ValueError("num_classes must be an integer >= 2; got %r" % (num_classes,))
        if not 0.0 < float(epsilon) < 1.0:
            raise ValueError("epsilon must lie in (0, 1); got %r" % (epsilon,))
        self.num_classes = int(num_classes)
        self.epsilon = float(epsilon)

    @property
    def num_latent(self):
        return self.num_classes

    def _log_hit_miss(self):
        return math.log1p(-self.epsilon), math.log(self.epsilon / (self.num_classes - 1))

    def check_labels(self, Y):
        """Y [n, 1] (or [n]) must hold integers in [0, num_classes): ValueError otherwise."""
        Y = torch.as_tensor(Y)
        if not (Y.dim() == 1 or (Y.dim() == 2 and Y.shape[1] == 1)):
            raise ValueError("MultiClass expects one column of class labels; got shape %s" % (tuple(Y.shape),))
        if Y.numel() and not bool(((Y >= 0) & (Y < self.num_classes) & (Y == torch.floor(Y))).all()):
            raise ValueError("MultiClass labels must be integers in [0, %d)" % self.num_classes)

    def _native(self, t):
        from .models import sparse_gpr
        return sparse_gpr.NATIVE_EXPECTATION and t.is_cuda and type(self) is MultiClass

    def _check_marginals(self, f_mean, f_var):
        if f_mean.dim() != 2 or f_mean.shape[1] != self.num_classes:
            raise ValueError("expect means of shape [n, %d]; got %s" % (self.num_classes, tuple(f_mean.shape)))
        if f_var.dim() == 2:                                  # [n, 1], or one shared variance expanded over the columns
            f_var = f_var[:, 0]
        if f_var.shape != (f_mean.shape[0],):
            raise ValueError("expect one variance per row; got %s for %d rows" % (tuple(f_var.shape), f_mean.shape[0]))
        return f_var

    def _largest(self, f_mean, f_var, idx):
        """-> P [n]: the rule's probability that column idx[i] is the largest of row i."""
        x, w = gauss_hermite(self.num_gauss_hermite_points, f_mean.device)
        gap = (f_mean.gather(1, idx[:, None]) - f_mean) / torch.sqrt(f_var)[:, None]                 # [n, C]
        lp = _LogNdtr.apply(gap.unsqueeze(1) + (math.sqrt(2.0) * x)[None, :, None])                  # [n, H, C]
        own = torch.nn.functional.one_hot(idx, self.num_classes).bool().unsqueeze(1)
        return (torch.exp(lp.masked_fill(own, 0.0).sum(-1)) * w).sum(-1) * (1.0 / math.sqrt(math.pi))

    def variational_expectation(self, f_mean, f_var, labels):
        """<log p(y | f)> under N(f_mean [n, C], f_var [n]) summed over the rows (0-dim); labels [n] (or [n, 1])."""
        f_var = self._check_marginals(f_mean, f_var)
        labels = labels.reshape(-1)
        if labels.shape[0] != f_mean.shape[0]:
            raise ValueError("Targets (%i) and q(f) (%i rows) have mismatch in size" % (labels.shape[0], f_mean.shape[0]))
        if self._native(f_mean):
            from .models import sparse_gpr
            return sparse_gpr._RobustMaxNode.apply(self.epsilon, self.num_gauss_hermite_points, f_mean, f_var, labels)
        hit, miss = self._log_hit_miss()
        P = self._largest(f_mean, f_var, labels.long())
        return (P * hit + (1.0 - P) * miss).sum()

    def predict_mean_variance(self, mean_f, var_f):
        """-> (p [n, C], p (1 - p)) with p[:, c] = (1 - epsilon) P_c + epsilon / (C - 1) (1 - P_c), P_c the rule's probability
        that column c is the largest.  The C probabilities of a row add to 1 only to the accuracy of the rule (exactly for
        C = 2, where the rule is symmetric); they are returned as they are, not renormalised."""
        var_f = self._check_marginals(mean_f, var_f)
        if self._native(mean_f):
            from . import _ops
            x, w = gauss_hermite(self.num_gauss_hermite_points, mean_f.device)
            p = _ops.lik_robustmax_probs(mean_f.detach(), var_f.detach(), self.epsilon, x, w)
        else:
            miss = self.epsilon / (self.num_classes - 1)
            cols = []
            for c in range(self.num_classes):
                P = self._largest(mean_f, var_f, torch.full((mean_f.shape[0],), c, dtype=torch.long, device=mean_f.device))
                cols.append((1.0 - self.epsilon) * P + miss * (1.0 - P))
            p = torch.stack(cols, 1)
        return p, p * (1.0 - p)

    def logp(self, F, Y):
        """the pointwise definition: F [..., C], Y [...] or [..., 1] -> log p(y | f) of Y's shape."""
        hit, miss = self._log_hit_miss()
        labels = Y.reshape(F.shape[:-1]).long()
        lp = torch.where(torch.argmax(F, -1) == labels, torch.full_like(F[..., 0], hit), torch.full_like(F[..., 0], miss))
        return lp.reshape(Y.shape)

    def propagate_log(self, qf, targets):
        raise NotImplementedError("MultiClass couples the latent columns of a row: propagate_log's contract is one column at a "
                                  "time; use variational_expectation(f_mean [n, C], f_var [n], labels [n])")


class Poisson(_NonGaussian):
    """Counts y with rate exp(f) (log link): logp = y f - exp(f) - lgamma(y + 1).  Everything is CLOSED FORM: the expectation
    y mu - exp(mu + v / 2) - lgamma(y + 1), the predictive mean exp(mu + v / 2) and variance mean + (e^v - 1) mean^2."""

    def logp(self, F, Y):
        return Y * F - torch.exp(F) - torch.lgamma(Y + 1.0)

    def logp_derivatives(self, F, Y):
        m = torch.exp(F)
        return Y * F - m - torch.lgamma(Y + 1.0), Y - m, m, -m

    def conditional_mean(self, F):
        return torch.exp(F)

    def conditional_variance(self, F):
        return torch.exp(F)

    def propagate_log(self, qf, targets):
        mu, v = _check_gaussian(qf, targets)
        y = targets.reshape(mu.shape)
        return (y * mu - torch.exp(mu + 0.5 * v) - torch.lgamma(y + 1.0)).sum()

    def predict_mean_variance(self, mean_f, var_f):
        mean = torch.exp(mean_f + 0.5 * var_f)
        return mean, mean + torch.expm1(var_f) * mean * mean


class StudentT(_NonGaussian):
    """y = f + scale * t_df: heavy-tailed noise for outlier-robust regression.  `scale` is a positive Param, `df` a fixed float
    > 2 (so that the variance exists).  The expectation of logp goes by quadrature; the predictive mean mu and variance
    v + scale^2 df / (df - 2) are CLOSED FORM."""

    def __init__(self, df=3.0, scale=1.0):
        super().__init__()
        if not float(df) > 2.0:
            raise ValueError("df must be > 2; got %r" % (df,))
        self.df = float(df)
        self.scale = Param(torch.tensor([float(scale)], dtype=torch_dtype), transform=DefaultPositiveTransform())

    def _logp_of_residual(self, r, s2):
        nu = self.df
        const = math.lgamma(0.5 * (nu + 1.0)) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi)
        return const - 0.5 * torch.log(s2) - 0.5 * (nu + 1.0) * torch.log1p(r * r / (nu * s2))

    def logp(self, F, Y):
        s = self.scale.transform()
        return self._logp_of_residual(Y - F, s * s)

    def propagate_log(self, qf, targets):
        """the rule with the residual formed as (y - mu) - sqrt(2 v) x_h: where a target is close to its mean and v is small,
        y - f_h rounded from f_h = mu + sqrt(2 v) x_h would lose what y - mu keeps exactly (csrc/lik.hip does the same)."""
        mu, v = _check_gaussian(qf, targets)
        x, w = gauss_hermite(self.num_gauss_hermite_points, mu.device)
        r = (targets.reshape(mu.shape) - mu).unsqueeze(-1) - torch.sqrt(2.0 * v).unsqueeze(-1) * x
        s = self.scale.transform()
        return (self._logp_of_residual(r, s * s) * (w * (1.0 / math.sqrt(math.pi)))).sum(-1).sum()

    def conditional_mean(self, F):
        return F

    def conditional_variance(self, F):
        s = self.scale.transform()
        return (s * s * (self.df / (self.df - 2.0))).expand_as(F)

    def predict_mean_variance(self, mean_f, var_f):
        s = self.scale.transform()
        return mean_f, var_f + (s * s * (self.df / (self.df - 2.0))).expand_as(var_f)
