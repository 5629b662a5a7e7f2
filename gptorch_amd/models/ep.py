"""
Exact GP classification by expectation propagation (Rasmussen & Williams ch. 3.6 and 5.5.2; Kuss & Rasmussen 2005) over the
native factorisation pipeline -- the approximation whose predictive probabilities and evidence are the accurate ones for a
Bernoulli likelihood, where Laplace's (models/laplace.py) are under-confident.  The reference has no counterpart: its Likelihood
leaves the non-conjugate case as a TODO (gptorch/likelihoods.py:47-78).

Notation: labels t = 2y - 1, m = mean_function(X), sites t_i(f_i) prop. to exp(nu_i f_i - 1/2 tau_i f_i^2),
s = sqrt(max(tau, W_FLOOR)), w = nu - tau m.

One sweep (PARALLEL EP: every site is updated from the same posterior; one host read per sweep):

    B = I + diag(s) K diag(s) = L L^T                   gpn_laplace_system + the MFMA Cholesky, L^-1 (s K w) riding along as the extra row
    a = w - s B^-1 (s K w),   mu = m + K a              gpn_laplace_matvec, gpn_backsub: LaplaceGP's Newton step with another right-hand side
    sigma2_i = Sigma_ii = (1 / s_i) sum_j K_ij s_j Binv_ji            L^-T, Binv = L^-T L^-1, gpn_laplace_diag (the row dot that does not cancel)
    cavity  tau_c = 1 / sigma2 - tau,  nu_c = mu / sigma2 - nu
    tilted moments  log Z^, mu_hat, s2_hat of  p(y_i | f) N(f | nu_c / tau_c, 1 / tau_c)
    update  tau <- max(tau + rho (1 / s2_hat - tau_c - tau), 0),   nu <- nu + rho (mu_hat / s2_hat - nu_c - nu)       rho = damping

The last three lines, the site part of the evidence and the stopping statistics are ONE entry point, gpn_ep_sites (csrc/ep.hip).
The search stops when change = max(|delta tau|, |delta nu|) (the UNDAMPED differences) <= ep_tol (1 + max(|tau|, |nu|)); it also
stops, recorded as ep_stats["stalled"], when the change is below STALL_BELOW of that scale and is below neither of the TWO sweeps
before (the rounding floor; two, because a damped sweep may converge with alternating sign, its change falling every other sweep: a
comparison with the last sweep alone ends such a search at 1e-8); it raises RuntimeError after max_sweeps.  Then ONE more assembly
and factorisation at the sites found, with the posterior, the cavity and the moments but no update: the evidence, its gradients
and the prediction state all belong to the same (tau, nu).

    log Z_EP = sum_i e_i + 1/2 w^T K a - sum log L_ii
    e_i = log Z^_i + 1/2 log1p(tau_i / tau_c) + 1/2 (tau_c c (tau_i c - 2 w_i) - w_i^2) / (tau_c + tau_i),   c = nu_c / tau_c - m_i

which is sum log Z~_i + log N(mu~ | m, K + Sigma~) (R&W eq. 3.65; mu~ = nu / tau) rearranged as R&W eqs. 3.73-3.74 with mu~ - m in
the place of mu~: no term divides by tau_i, a site with tau_i = 0 contributes its finite limit.

Gradients at the fixed point (R&W eq. 5.27: no implicit term), with R = diag(s) B^-1 diag(s):

    dlog Z_EP/dtheta = sum_ij G_ij dK_ij/dtheta,  G = 1/2 a a^T - 1/2 R       (gpn_laplace_grad with u = 0)
    dlog Z_EP/dm = a

Likelihoods: Bernoulli("probit") (closed-form moments, R&W eqs. 3.58 and 3.82) and Bernoulli("logit") (the three moments by the
likelihood's own Gauss-Hermite rule of num_gauss_hermite_points nodes: that rule is the model's definition, as it is for
propagate_log).  Prediction is LaplaceGP's (laplace.SearchedGP._predict) over (a, s, the factor) of the converged sites.

Lock step: equal-shape EPGP models handed to multi_start_optimize / batched_log_likelihood / batched_loss_and_grad /
batched_factorise run their searches, evidences and gradients as one group (models/_ep_lockstep.py, _lockstep._ep_groups), every
model's numbers bit-identical to its own evaluation; a group's models share the kernel kind, the link, X's shape, ARD or not and,
for logit, the number of Gauss-Hermite nodes.

Out of scope: optimize(capture=True) (the search reads the host; under multi_start_optimize(capture=True) EPGP models keep their
own optimize()), DistGPR, ragged groups, sequential (rank-one) EP, Poisson and other likelihoods, composite kernels, dy > 1.
"""
import torch

from .. import _backward, _ops, kernels, likelihoods
from .._native import LIK_LOGIT, LIK_PROBIT, NativeError
from ._site_lockstep import Evidence
from .laplace import SearchedGP, SearchEvidence, W_FLOOR, _dot, _factor_system, _inverse_at

STALL_BELOW = 1e-6         # a change that no longer decreases counts as a stall only below this fraction of the sites' scale


class _Sites:
    """what one EP search leaves: the sites, a, K a, s, the factor of B at the sites, the evidence and the search's statistics."""
    __slots__ = ("tau", "nu", "a", "Ka", "s", "mu", "sigma2", "mu_hat", "s2_hat", "factor", "generation", "evidence", "sweeps", "stalled")


def _posterior(kind, X, m, var, ls, tau, nu, factor, work):
    """steps 1-3 of a sweep at the sites (tau, nu) -> (s, a, K a, mu, sigma2); the factor buffer holds L afterwards."""
    s = torch.sqrt(torch.clamp(tau, min=W_FLOOR))
    w = nu - tau * m
    _factor_system(kind, X, var, ls, s, factor, rhs=s * _ops.laplace_matvec(kind, X, var, ls, w, work=work))
    a = w - s * _ops.backsub(factor)[0]
    Ka = _ops.laplace_matvec(kind, X, var, ls, a, work=work)
    Binv = _backward._kinv_lower(factor, _backward._upper_inverse(factor))
    sigma2 = _ops.laplace_diag(kind, X, var, ls, s, Binv, work=work)
    return s, a, Ka, m + Ka, sigma2


def find_sites(kind, lik_kind, X, y, m, var, ls, rule=(None, None), sites0=None, factor=None, ep_tol=1e-10, max_sweeps=200, damping=0.8):
    """The search described in the module docstring -> _Sites.  y, m [n]; rule: (nodes, weights) of the logit link;
    sites0: (tau, nu) to start from (None: zero)."""
    n = X.shape[0]
    dev = X.device
    if factor is None or factor.n != n or factor.e != 1 or factor.device != dev:
        factor = _ops.Factor(n, 1, dev)
    work = _ops._rows_work(n, dev, None)
    if sites0 is None:
        tau = torch.zeros(n, dtype=torch.float64, device=dev)
        nu = torch.zeros_like(tau)
    else:
        tau, nu = sites0[0].detach(), sites0[1].detach()            # (never written in place)
    sweeps, stalled, before = 0, False, []
    while True:
        if sweeps >= max_sweeps:
            raise RuntimeError("EPGP: the sites did not converge in %d sweeps (ep_tol = %g, damping = %g)" % (max_sweeps, ep_tol, damping))
        _, _, _, mu, sigma2 = _posterior(kind, X, m, var, ls, tau, nu, factor, work)
        tau, nu, _, _, _, stats = _ops.ep_sites(lik_kind, y, m, mu, sigma2, tau, nu, damping, *rule, want_moments=False)
        sweeps += 1
        # the sweep's ONE host read: the statistics and the factorisation's info word
        _, _, dtau, dnu, mtau, mnu, info = torch.cat([stats, factor.info.double()]).tolist()
        if info != 0:
            raise NativeError("EPGP: the factorisation of B = I + S^1/2 K S^1/2 reported info = %d (its eigenvalues are >= 1: "
                              "a non-finite parameter or input?)" % int(info))
        change, scale = max(dtau, dnu), 1.0 + max(mtau, mnu)
        if change <= ep_tol * scale:
            break
        if len(before) == 2 and change <= STALL_BELOW * scale and change >= max(before):
            stalled = True
            break
        before = (before + [change])[-2:]
    st = _Sites()
    st.tau, st.nu = tau, nu
    st.s, st.a, st.Ka, st.mu, st.sigma2 = _posterior(kind, X, m, var, ls, tau, nu, factor, work)       # the factor AT the sites
    _, _, _, st.mu_hat, st.s2_hat, stats = _ops.ep_sites(lik_kind, y, m, st.mu, st.sigma2, tau, nu, damping, *rule, moments_only=True)
    terms = factor.lml_terms()
    if int(factor.info.item()) != 0:
        raise NativeError("EPGP: the factorisation at the converged sites reported info = %d" % int(factor.info.item()))
    st.evidence = stats[1] + 0.5 * _dot(nu - tau * m, st.Ka) - terms[0]
    st.factor, st.generation = factor, factor.generation
    st.sweeps, st.stalled = sweeps, stalled
    return st


def _evidence_gradients(kind, X, var, ls, st):
    """the closed form of the module docstring at one search's sites -> (g [1 + nls] = dlog Z_EP/d(variance, length_scales), None:
    there is no u)"""
    _, Binv = _inverse_at(kind, X, var, ls, st)
    zero = torch.zeros_like(st.a)
    return _ops.laplace_grad(kind, X, var, ls, st.s, Binv, st.a, zero, zero), None


class EPEvidence(SearchEvidence):
    """log Z_EP: the EP search in the forward, the closed form of the module docstring in the backward"""
    family = Evidence(value=lambda st: st.evidence, gradients=_evidence_gradients, mean_gradient=lambda st, _u: st.a)


class EPGP(SearchedGP):
    """EPGP(x, y, kernel, likelihood): the exact GP under Bernoulli("probit" | "logit") labels, its hyper-parameters fitted on
    the evidence of expectation propagation (see the module docstring).  GPU only.

    ep_tol, max_sweeps, damping: the stopping rule and the step of the parallel sweeps.  warm_start (default on): a search starts
    at the previous evaluation's sites when the shapes match; reset_sites() drops them.  ep_stats: {"sweeps", "stalled"} of the
    last search."""
    _tag = "ep"

    def __init__(self, x, y, kernel, likelihood, mean_function=None, name="ep_gp"):
        if not (isinstance(kernel, kernels.Stationary) and kernel._kind is not None):
            raise NotImplementedError("EPGP assembles B = I + S^1/2 K S^1/2 from a native stationary kernel (Rbf, Matern52, "
                                      "Matern32, Exp, Periodic); got %s -- composite, linear and static kernels: SVGP with Z = X"
                                      % type(kernel).__name__)
        if isinstance(likelihood, likelihoods.Gaussian) or likelihood is None:
            raise ValueError("a Gaussian likelihood is conjugate: use GPR, whose evidence is exact")
        if isinstance(likelihood, likelihoods.StudentT):
            raise NotImplementedError("StudentT is not log-concave (a site precision may be negative and B indefinite): use SVGP")
        if type(likelihood) is not likelihoods.Bernoulli:
            raise NotImplementedError("EPGP takes Bernoulli('probit' | 'logit'); got %s -- LaplaceGP takes Poisson, SVGP takes any "
                                      "likelihood with a logp" % type(likelihood).__name__)
        self._lik_kind = LIK_PROBIT if likelihood.link == "probit" else LIK_LOGIT
        if y.ndim != 2 or y.shape[1] != 1:
            raise ValueError("EPGP takes one output column, Y [N, 1]; got %s -- fit one model per column" % (tuple(y.shape),))
        super().__init__(x, y, kernel, likelihood, mean_function, name)
        self.ep_tol = 1e-10
        self.max_sweeps = 200
        self.damping = 0.8
        self.warm_start = True
        self.ep_stats = {"sweeps": 0, "stalled": False}
        self._holder = {}
        self._sites = None
        self._predict_cache = None
        self._predict_calls = 0

    def reset_sites(self):
        """forget the previous sites: the next evaluation starts its search at tau = nu = 0."""
        self._sites = None

    def _start(self, n):
        s = self._sites
        return s if (self.warm_start and s is not None and s[0].numel() == n and s[0].device == self.X.device) else None

    def _rule(self, device):
        if self._lik_kind == LIK_PROBIT:
            return (None, None)
        return likelihoods.gauss_hermite(self.likelihood.num_gauss_hermite_points, device)

    def _search(self, kind, lik_kind, X, y, m, var, ls, factor=None):
        return find_sites(kind, lik_kind, X, y, m, var, ls, rule=self._rule(X.device), sites0=self._start(X.shape[0]), factor=factor,
                          ep_tol=self.ep_tol, max_sweeps=self.max_sweeps, damping=self.damping)

    def _remember(self, st):
        self._sites = (st.tau, st.nu)
        self.ep_stats = {"sweeps": st.sweeps, "stalled": st.stalled}

    def log_likelihood(self, x=None, y=None):
        """log Z_EP, expectation propagation's approximation of the evidence; a tensor of shape (1,)."""
        x = x if x is not None else self.X
        y = y if y is not None else self.Y
        if not x.shape[0] == y.shape[0]:
            raise ValueError("X and Y must have same # data.")
        k = self.kernel
        return EPEvidence.apply(x, y, self.mean_function(x), k.variance.transform(), k.length_scales.transform(), k._kind,
                                self._lik_kind, self)
