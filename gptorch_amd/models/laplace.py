"""
Exact GP classification and count regression by Laplace's approximation (Rasmussen & Williams ch. 3 and 5.5) over the native
factorisation pipeline.  The reference has no counterpart: its Likelihood leaves the non-conjugate case as a TODO
(gptorch/likelihoods.py:47-78).

With lp_i = log p(y_i | f_i), d1 = dlp/df, W = -d2lp/df2, d3 = d3lp/df3, s = sqrt(W) and m = mean_function(X), the posterior
mode is parameterised by a: f = m + K a (at the mode a = d1), and

    psi(a) = sum lp(m + K a) - 1/2 a^T K a                       the objective of the mode search
    B = I + diag(s) K diag(s) = L L^T                            eigenvalues >= 1: no jitter ladder
    b = W (f - m) + d1,   a+ = b - s B^-1 (s K b)                one Newton step
    log q(y | theta) = psi(a^) - sum log L_ii                    the approximate evidence, L the factor AT the mode

One Newton step is: gpn_lik_derivs (pointwise), gpn_laplace_matvec (K b, matrix-free), gpn_laplace_system (B assembled straight
into the lower tiles of the factor buffer; K is never stored), the MFMA Cholesky with L^-1 (s K b) riding along as the extra
row, gpn_backsub (L^-T of that row), gpn_laplace_matvec (K a+).  K a is linear in a, so a step of length t needs no further
product: K (a + t (a+ - a)) is a blend of the two products held.  The step is halved while psi would decrease (at most
MAX_HALVINGS times); plain Newton overshoots for Poisson counts.  The search stops after the first step with
max |delta f| <= newton_tol (1 + max |f|) and raises RuntimeError after max_newton_iter steps.  One host read per trial step
(psi, the two maxima and the factorisation's info word together).  Then ONE more factorisation at the mode itself gives L.

Evidence gradients (closed form), with Binv = B^-1, R = diag(s) Binv diag(s):

    Sigma_ii = [(K^-1 + W)^-1]_ii = (1 / s_i) sum_j K_ij s_j Binv_ji      (gpn_laplace_diag: a row dot that does not cancel, where
                                                                           the textbook (1 - Binv_ii) / W_i does)
    s2 = 1/2 Sigma_ii d3                    = d(-1/2 log|B|)/df_i         (the sign of R&W eq. 5.23 is the subject of errata)
    u = s2 - R K s2                         = (I + W K)^-1 s2
    dlog q/dtheta = sum_ij G_ij dK_ij/dtheta,  G = 1/2 a a^T - 1/2 R + 1/2 (u d1^T + d1 u^T)      (gpn_laplace_grad)
    dlog q/dm = d1 + u

W is floored at the smallest normal fp64 number (2.2e-308) before the square root, so that 1 / s is finite where a likelihood
has saturated (a Bernoulli point 38 standard deviations on the right side of the boundary).

Prediction: mean_f = m(x*) + K(x*, X) a^, cov_f = K(x*, x*) - V^T V with V = L^-1 diag(s) K(X, x*); predict_y hands the
marginals to likelihood.predict_mean_variance (diag=False raises: a non-Gaussian likelihood has no predictive covariance).
The mode, s and the factor are kept between predictions (GPModel._cached_state).

Restarts and folds: equal-shape LaplaceGP models handed to batched_log_likelihood / batched_loss_and_grad / multi_start_optimize /
batched_factorise run their searches, evidences, gradients and prediction states in LOCK STEP (models/_laplace_lockstep.py), every
number bit-identical to the model's own evaluation here.

Out of scope: composite kernels, dy > 1, Student-t (not log-concave: W may be negative and B indefinite), ragged (unequal-N)
lock-step groups, optimize(capture=True) (the search reads the host), DistGPR.  Expectation propagation, the more accurate
approximation for Bernoulli labels, is models.EPGP (models/ep.py), which runs on these kernels and shares _predict below.
"""
import sys

import torch

from .. import _backward, _ops, kernels, likelihoods
from .._native import LIK_LOGIT, LIK_POISSON, LIK_PROBIT, NativeError
from ._site_lockstep import Evidence
from .base import GPModel

MAX_HALVINGS = 10
PSI_SLACK = 1e-10          # a trial step "decreases" psi when psi_t < psi - PSI_SLACK (1 + |psi|): rounding of the n-term sums is no decrease
W_FLOOR = sys.float_info.min


class _Mode:
    """what one mode search leaves: a^, K a^, f^, sum lp, d1, W, d3, s at the mode, the factor of B there, sum log L_ii."""
    __slots__ = ("a", "Ka", "f", "value", "d1", "W", "d3", "s", "factor", "generation", "sum_log_diag", "steps", "halvings")


def _dot(x, y):
    return _ops.dot2d(x.reshape(1, -1), y.reshape(1, -1))


def _factor_system(kind, X, var, ls, s, factor, rhs=None):
    """B = I + diag(s) K diag(s) assembled into the factor buffer and factorised, rhs [n] forward-substituted on the way;
    nothing is read back."""
    _ops.laplace_system(kind, X, var, ls, s, factor.A, factor.ld)
    factor.pack_rhs((torch.zeros_like(s) if rhs is None else rhs).reshape(-1, 1))
    factor.potrf(check=False)


def find_mode(kind, lik_kind, X, y, m, var, ls, a0=None, factor=None, newton_tol=1e-8, max_newton_iter=50):
    """The Newton search described in the module docstring -> _Mode.  y, m [n]; a0: the start (None: zero)."""
    n = X.shape[0]
    dev = X.device
    if factor is None or factor.n != n or factor.e != 1 or factor.device != dev:
        factor = _ops.Factor(n, 1, dev)
    work = _ops._rows_work(n, dev, None)

    def kv(v):
        return _ops.laplace_matvec(kind, X, var, ls, v, work=work)

    if a0 is None:
        a = torch.zeros(n, dtype=torch.float64, device=dev)
        Ka = torch.zeros_like(a)
    else:
        a = a0.detach().clone()
        Ka = kv(a)
    f = m + Ka
    value, d1, W, _ = _ops.lik_derivs(lik_kind, f, y, want_d3=False)
    psi = value - 0.5 * _dot(a, Ka)
    steps = halvings = 0
    while True:
        if steps >= max_newton_iter:
            raise RuntimeError("LaplaceGP: the mode search did not converge in %d Newton steps (newton_tol = %g)"
                               % (max_newton_iter, newton_tol))
        s = torch.sqrt(torch.clamp(W, min=W_FLOOR))
        b = W * Ka + d1
        _factor_system(kind, X, var, ls, s, factor, rhs=s * kv(b))
        a_new = b - s * _ops.backsub(factor)[0]
        Ka_new = kv(a_new)
        t = 1.0
        for h in range(MAX_HALVINGS + 1):
            a_t = a_new if t == 1.0 else a + t * (a_new - a)
            Ka_t = Ka_new if t == 1.0 else Ka + t * (Ka_new - Ka)
            f_t = m + Ka_t
            value_t, d1_t, W_t, _ = _ops.lik_derivs(lik_kind, f_t, y, want_d3=False)
            psi_t = value_t - 0.5 * _dot(a_t, Ka_t)
            # the step's ONE host read: psi before and after, the two maxima of the stopping rule, the factorisation's info
            got, was, max_df, max_f, info = torch.stack([psi_t, psi, (f_t - f).abs().max(), f_t.abs().max(), factor.info[0].double()]).tolist()
            if info != 0:
                raise NativeError("LaplaceGP: the factorisation of B = I + W^1/2 K W^1/2 reported info = %d (for a positive "
                                  "semi-definite K its eigenvalues are >= 1: a non-finite parameter or input -- or a kernel that "
                                  "is not positive semi-definite, as Periodic is from two input dimensions on?)" % int(info))
            if got >= was - PSI_SLACK * (1.0 + abs(was)) or h == MAX_HALVINGS:       # (NaN / -inf: not accepted, halve)
                break
            t *= 0.5
            halvings += 1
        a, Ka, f, value, d1, W, psi = a_t, Ka_t, f_t, value_t, d1_t, W_t, psi_t
        steps += 1
        if max_df <= newton_tol * (1.0 + max_f):
            break
    mode = _Mode()
    mode.a, mode.Ka, mode.f = a, Ka, f
    mode.value, mode.d1, mode.W, mode.d3 = _ops.lik_derivs(lik_kind, f, y)
    mode.s = torch.sqrt(torch.clamp(mode.W, min=W_FLOOR))
    _factor_system(kind, X, var, ls, mode.s, factor)                                # the factor AT the mode
    terms = factor.lml_terms()
    if int(factor.info.item()) != 0:
        raise NativeError("LaplaceGP: the factorisation at the mode reported info = %d" % int(factor.info.item()))
    mode.factor, mode.generation, mode.sum_log_diag = factor, factor.generation, terms[0]
    mode.steps, mode.halvings = steps, halvings
    return mode


def _solve_b(factor, w):
    """B^-1 w [n] with the factor held: the forward half as a one-row right-solve, the back-substitution on the extra row."""
    n = factor.n
    row = _ops.padded_like_factor(factor, 1)
    row[0, :n] = w
    factor.solve_right_lt(row, 1)
    factor.A[n, :n] = row[0, :n]
    return _ops.backsub(factor)[0]


def _inverse_at(kind, X, var, ls, state):
    """(the factor of B at a search's state, B^-1 from it)"""
    f = state.factor
    if f.generation != state.generation:
        # the model's reusable buffer was refactorised by a later forward: rebuild this node's factor privately
        f = _ops.Factor(f.n, 1, f.device)
        _factor_system(kind, X, var, ls, state.s, f)
    return f, _backward._kinv_lower(f, _backward._upper_inverse(f))


def _evidence_gradients(kind, X, var, ls, mode):
    """the closed form of the module docstring at one mode -> (g [1 + nls] = dlog q/d(variance, length_scales), u [n])"""
    f, Binv = _inverse_at(kind, X, var, ls, mode)
    sigma = _ops.laplace_diag(kind, X, var, ls, mode.s, Binv)
    s2 = 0.5 * sigma * mode.d3
    u = s2 - mode.s * _solve_b(f, mode.s * _ops.laplace_matvec(kind, X, var, ls, s2))
    return _ops.laplace_grad(kind, X, var, ls, mode.s, Binv, mode.a, u, mode.d1), u


class SearchEvidence(torch.autograd.Function):
    """one model's approximate evidence as ONE autograd node: the owner's search in the forward, the family's closed form in the
    backward; a family's node is a subclass that sets `family` (a _site_lockstep.Evidence; forward and backward, static methods,
    find it through ctx._forward_cls: the class whose apply() was called, which torch.autograd sets on every node's class).  Inputs: the points, the targets [n, 1],
    m = mean_function(X) [n, 1], the CONSTRAINED variance and length-scales, the kernel and likelihood kinds, the model; gradients
    for m, variance and length-scales."""
    family = None

    @staticmethod
    def forward(ctx, X, Y, m, variance, length_scales, kind, lik_kind, owner):
        state = owner._search(kind, lik_kind, X, Y.detach().reshape(-1), m.detach().reshape(-1), variance.detach(), length_scales.detach(),
                              factor=owner._holder.get("factor"))
        owner._holder["factor"] = state.factor
        owner._remember(state)
        ctx.kind, ctx.state = kind, state
        ctx.save_for_backward(X, variance, length_scales)
        return ctx._forward_cls.family.value(state).reshape(1)

    @staticmethod
    def backward(ctx, grad_out):
        family = ctx._forward_cls.family
        X, variance, length_scales = ctx.saved_tensors
        kind, state = ctx.kind, ctx.state
        n = state.factor.n
        g, u = family.gradients(kind, X, variance.detach(), length_scales.detach(), state)
        go = grad_out.reshape(())
        nls = length_scales.numel()
        return (None, None, (go * family.mean_gradient(state, u)).reshape(n, 1) if ctx.needs_input_grad[2] else None,
                (go * g[0:1]).reshape(variance.shape), (go * g[1:1 + nls]).reshape(length_scales.shape), None, None, None)


class LaplaceEvidence(SearchEvidence):
    """log q(y | theta): the Newton loop in the forward, the closed form of the module docstring in the backward"""
    family = Evidence(value=lambda mode: mode.value - 0.5 * _dot(mode.a, mode.Ka) - mode.sum_log_diag, gradients=_evidence_gradients,
                      mean_gradient=lambda mode, u: mode.d1 + u)


class SearchedGP(GPModel):
    """what LaplaceGP and EPGP (models/ep.py) share: q(f* | y) from what a search leaves -- a, s and the factor of
    B = I + diag(s) K diag(s).  A subclass gives _tag (it names the cached state), _search, _start and _remember."""

    def _mode_for_predict(self, x):
        """the state _predict starts from, a in the factor's extra row: the operand of the predictive mean"""
        k = self.kernel
        with torch.no_grad():
            var, ls = k.variance.transform(), k.length_scales.transform()

            def build():
                state = self._search(k._kind, self._lik_kind, x, self.Y.reshape(-1), self.mean_function(x).reshape(-1), var, ls)
                self._remember(state)
                state.factor.A[state.factor.n, :state.factor.n] = state.a
                return state

            state = self._cached_state((self._tag, k._kind), x, build)
            self._predict_calls += 1
        return state, var, ls

    def _predict(self, x_new, diag=True, x=None):
        """q(f* | y): mean [n*, 1]; var [n*, 1] (diag) or cov [n*, n*]."""
        x = x if x is not None else self.X
        mode, var, ls = self._mode_for_predict(x)
        k, f = self.kernel, mode.factor
        n, ns = f.n, x_new.shape[0]
        with torch.no_grad():
            Bt = _ops.padded_like_factor(f, ns)
            _ops.kernel_matrix(k._kind, x_new, x, var, ls, out=Bt, ldk=f.ld)                  # K(x*, X)
            kpad = _ops.round_up(n, 16)
            mean = _ops.gemm_nt(Bt, f.A[n:], ns, 1, kpad) + self.mean_function(x_new)        # K(x*, X) a^ + m(x*)
            Bt[:ns, :n] *= mode.s                                                            # K(x*, X) diag(s)
            f.solve_right_lt(Bt, ns)                                                         # V^T = K(x*, X) diag(s) L^-T
            if diag:
                return mean, (var.expand(ns) - _ops.row_sumsq(Bt, ns, n))[:, None]
            cov = _ops.kernel_matrix(k._kind, x_new, None, var, ls)
            _ops.gemm_nt(Bt, Bt, ns, ns, kpad, alpha=-1.0, beta=1.0, C=cov)
            return mean, cov


class LaplaceGP(SearchedGP):
    """LaplaceGP(x, y, kernel, likelihood): the exact GP under Bernoulli("probit" | "logit") labels or Poisson counts, its
    hyper-parameters fitted on Laplace's approximate evidence (see the module docstring).  GPU only.

    newton_tol, max_newton_iter: the stopping rule of the mode search.  warm_start (default on): a search starts at the
    previous evaluation's mode when the shapes match; reset_mode() drops it.  newton_stats: {"steps", "halvings"} of the
    last search."""
    _tag = "laplace"

    def __init__(self, x, y, kernel, likelihood, mean_function=None, name="laplace_gp"):
        if not (isinstance(kernel, kernels.Stationary) and kernel._kind is not None):
            raise NotImplementedError("LaplaceGP assembles B = I + W^1/2 K W^1/2 from a native stationary kernel (Rbf, Matern52, "
                                      "Matern32, Exp, Periodic); got %s -- composite, linear and static kernels: SVGP with Z = X"
                                      % type(kernel).__name__)
        if isinstance(likelihood, likelihoods.Gaussian) or likelihood is None:
            raise ValueError("a Gaussian likelihood is conjugate: use GPR, whose evidence is exact")
        if isinstance(likelihood, likelihoods.StudentT):
            raise NotImplementedError("StudentT is not log-concave (W may be negative and B indefinite): use SVGP")
        if type(likelihood) is likelihoods.Bernoulli:
            self._lik_kind = LIK_PROBIT if likelihood.link == "probit" else LIK_LOGIT
        elif type(likelihood) is likelihoods.Poisson:
            self._lik_kind = LIK_POISSON
        else:
            raise NotImplementedError("LaplaceGP takes Bernoulli('probit' | 'logit') and Poisson; got %s -- SVGP takes any likelihood "
                                      "with a logp" % type(likelihood).__name__)
        if y.ndim != 2 or y.shape[1] != 1:
            raise ValueError("LaplaceGP takes one output column, Y [N, 1]; got %s -- fit one model per column" % (tuple(y.shape),))
        super().__init__(x, y, kernel, likelihood, mean_function, name)
        self.newton_tol = 1e-8
        self.max_newton_iter = 50
        self.warm_start = True
        self.newton_stats = {"steps": 0, "halvings": 0}
        self._holder = {}
        self._mode_a = None
        self._predict_cache = None
        self._predict_calls = 0

    def reset_mode(self):
        """forget the previous mode: the next evaluation starts its search at a = 0."""
        self._mode_a = None

    def _start(self, n):
        a = self._mode_a
        return a if (self.warm_start and a is not None and a.numel() == n and a.device == self.X.device) else None

    def _search(self, kind, lik_kind, X, y, m, var, ls, factor=None):
        return find_mode(kind, lik_kind, X, y, m, var, ls, a0=self._start(X.shape[0]), factor=factor, newton_tol=self.newton_tol,
                         max_newton_iter=self.max_newton_iter)

    def _remember(self, mode):
        self._mode_a = mode.a
        self.newton_stats = {"steps": mode.steps, "halvings": mode.halvings}

    def log_likelihood(self, x=None, y=None):
        """log q(y | theta), Laplace's approximation of the evidence; a tensor of shape (1,)."""
        x = x if x is not None else self.X
        y = y if y is not None else self.Y
        if not x.shape[0] == y.shape[0]:
            raise ValueError("X and Y must have same # data.")
        k = self.kernel
        return LaplaceEvidence.apply(x, y, self.mean_function(x), k.variance.transform(), k.length_scales.transform(), k._kind,
                                     self._lik_kind, self)
