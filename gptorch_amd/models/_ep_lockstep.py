"""
EPGP restarts and folds in LOCK STEP: the parallel-EP search of models/ep.py (find_sites), its evidence and its closed-form gradients
for B equal-shape models at once, every launch a strided-batch launch over the models (csrc/laplace.hip *_batched,
gpn_potrf_lower_batched, gpn_backsub_batched, gpn_lml_kinv_batched, gpn_ep_sites_batched).  A cold evaluation of one model is 17-18
sweeps of about ten small launches and one host read each; B restarts pay that chain B times, the group pays it once.

Every number a model receives is BIT-IDENTICAL to what its own log_likelihood() / loss().backward() / predict_f() computes:
  * per model the batched kernels run the single kernels' bodies on operands at a stride;
  * the elementwise torch expressions are ep._posterior's, on [k, n] stacks (a row's bits do not depend on the leading dimension);
  * every model keeps its own ep_tol, max_sweeps, damping (a device array: gpn_ep_sites_batched) and warm start, and applies
    find_sites' stopping rule and stall rule (the two-sweep memory, STALL_BELOW) to its own row of the ONE [k, 7] host read of a
    sweep (the six statistics and the factorisation's info);
  * a model that has converged or stalled leaves the search: the models still running are gathered (index_select) into a compact
    sub-batch that is factorised in the FIRST slots of the FactorBatch -- no kernel takes an index map, a finished model costs no
    further factorisation;
  * then ONE lock-step posterior at every model's sites, the moments without an update and sum log L_ii give the factors, the
    cavity moments and the evidence: all of the same (tau, nu), as find_sites leaves them.
A model whose factorisation reports info != 0, or that exhausts its max_sweeps, is replayed alone through find_sites, which raises
what it raises today: the whole call raises (models/_site_lockstep.py, which holds the scaffold this search shares with LaplaceGP's,
says why a group is never mixed).

Out of scope: ragged (unequal-N) groups, composite kernels, dy > 1, Poisson and Student-t, sequential (rank-one) EP, hipGraph capture,
DistGPR.
"""
import torch

from .. import _native, _ops
from . import _site_lockstep as site
from . import ep
from ._site_lockstep import _binv, _dots
from .ep import EPGP, STALL_BELOW
from .laplace import W_FLOOR

# counters for tests and tools/ep_lockstep_bench.py: lock-step searches, sweeps, host reads, and factorisations counted per MODEL
# (a sweep over k models adds k)
STATS = {"searches": 0, "sweeps": 0, "reads": 0, "factorisations": 0}

MAX_N = 8192        # the largest size measured (LAB 23, profiles/ep_lockstep.json): the lock-step median is below the sequential one in
#                     the cold and the warm column of every measured shape up to it; beyond it nothing is measured: sequential
MODEL = EPGP        # the class whose models these groups take


def supported(n):
    """sizes whose EPGP models are grouped: every measured shape up to MAX_N is faster in lock step, none beyond it is measured"""
    return 1 <= int(n) <= MAX_N


def per_model_bytes(n, nls=1):
    """what one model of a group holds at once, by the library's own sizes: its factor slot (matrix + leaf inverses), its block of
    gpn_lml_kinv_batched's workspace (B^-1 of a sweep and of the backward) and the gradient sweep's workspace"""
    lib = _native.lib()
    n = int(n)
    slot = 8 * int(lib.gpn_factor_rows(n, 1)) * int(lib.gpn_factor_ld(n, 1)) + int(lib.gpn_winv_bytes(n))
    return slot + int(lib.gpn_lml_kinv_batched_work_bytes(n, 1, 1)) + int(lib.gpn_laplace_grad_batched_work_bytes(n, int(nls), 1))


def _posteriors(kind, X, M, var, ls, tau, nu, fb, work):
    """ep._posterior for the k = tau.shape[0] models in the first slots of fb -> (s, a, K a, mu, sigma2), each [k, n]; the slots
    hold the factors afterwards."""
    k = tau.shape[0]
    s = torch.sqrt(torch.clamp(tau, min=W_FLOOR))
    w = nu - tau * M
    site._factor_systems(kind, X, var, ls, s, fb, STATS, rhs=s * _ops.laplace_matvec_batched(kind, X, var, ls, w, work=work))
    a = w - s * _ops.backsub_batched(fb, k)[:, 0]
    Ka = _ops.laplace_matvec_batched(kind, X, var, ls, a, work=work)
    binv, ld, stride = _binv(fb, k)
    sigma2 = _ops.laplace_diag_batched(kind, X, var, ls, s, binv, ld, stride, work=work)
    return s, a, Ka, M + Ka, sigma2


def _sites(kind, lik_kind, X, Y, M, var, ls, rule, starts, tols, max_sweeps, dampings, fb=None):
    """find_sites_batched -> the site.Stack of the B models' sites, with the [B, n] rows a"""
    everyone, fb, work = site.begin(X, Y, M, var, ls, fb)
    B, n, dev = len(everyone.act), X.shape[-2], X.device
    STATS["searches"] += 1

    def alone(b):
        """model b has failed: its own sequential search raises what the model alone raises"""
        e = everyone
        ep.find_sites(kind, lik_kind, e.X if e.X.dim() == 2 else e.X[b], e.Y if e.Y.dim() == 1 else e.Y[b], e.M[b], e.var[b:b + 1], e.ls[b],
                      rule=rule, sites0=starts[b], ep_tol=tols[b], max_sweeps=max_sweeps[b], damping=dampings[b])
        raise site.disagreement("EPGP", b)

    for b in range(B):
        # (the dampings travel as a device array that gpn_ep_sites_batched cannot check: a bad one meets gpn_ep_sites' own refusal)
        if max_sweeps[b] <= 0 or not 0.0 < float(dampings[b]) <= 1.0:
            alone(b)
    rho_all = torch.tensor([float(r) for r in dampings], dtype=torch.float64, device=dev)
    zero = torch.zeros(n, dtype=torch.float64, device=dev)
    tau = torch.stack([zero if start is None else start[0].detach().reshape(n) for start in starts])
    nu = torch.stack([zero if start is None else start[1].detach().reshape(n) for start in starts])
    run, rho = everyone, rho_all
    final = [None] * B                           # per model (its rows tau, nu at the sites found, stalled)
    sweeps, before = [0] * B, [[] for _ in range(B)]
    while run.act:
        k = len(run.act)
        STATS["sweeps"] += 1
        _, _, _, mu, sigma2 = _posteriors(kind, run.X, run.M, run.var, run.ls, tau, nu, fb, work)
        tau, nu, _, _, _, stats = _ops.ep_sites_batched(lik_kind, run.Y, run.M, mu, sigma2, tau, nu, rho, *rule, want_moments=False)
        # the sweep's ONE host read: every model's statistics and its factorisation's info word
        rows = torch.cat([stats, fb.info[:k].double()[:, None]], 1).tolist()
        STATS["reads"] += 1
        keep = []
        for j, b in enumerate(run.act):
            _, _, dtau, dnu, mtau, mnu, info = rows[j]
            sweeps[b] += 1
            if info != 0:
                alone(b)                         # (raises NativeError: info != 0)
            change, scale = max(dtau, dnu), 1.0 + max(mtau, mnu)
            if change <= tols[b] * scale:
                final[b] = (tau[j], nu[j], False)
            elif len(before[b]) == 2 and change <= STALL_BELOW * scale and change >= max(before[b]):
                final[b] = (tau[j], nu[j], True)
            elif sweeps[b] >= max_sweeps[b]:
                alone(b)                         # (raises RuntimeError: did not converge)
            else:
                before[b] = (before[b] + [change])[-2:]
                keep.append(j)
        run, (tau, nu, rho) = run.keep(keep, tau, nu, rho)
    # the posterior, the moments and the factor AT the sites, every model at once in its slot of the call
    e = everyone
    tau, nu = (torch.stack([found[i] for found in final]) for i in range(2))
    s, a, Ka, mu, sigma2 = _posteriors(kind, e.X, e.M, e.var, e.ls, tau, nu, fb, work)
    _, _, _, mu_hat, s2_hat, stats = _ops.ep_sites_batched(lik_kind, e.Y, e.M, mu, sigma2, tau, nu, rho_all, *rule, moments_only=True)
    sum_log_diag = site._sum_log_diags(fb, B)
    evidence = stats[:, 1] + 0.5 * _dots(nu - tau * e.M, Ka) - sum_log_diag
    found = []
    for b, info in enumerate(fb.info[:B].tolist()):
        if info != 0:
            alone(b)                             # (raises NativeError: the factorisation at the converged sites)
        one = ep._Sites()
        one.tau, one.nu, one.a, one.Ka, one.s = tau[b], nu[b], a[b], Ka[b], s[b]
        one.mu, one.sigma2, one.mu_hat, one.s2_hat = mu[b], sigma2[b], mu_hat[b], s2_hat[b]
        one.factor, one.generation, one.evidence = fb.factor(b), fb.generation, evidence[b]
        one.sweeps, one.stalled = sweeps[b], final[b][2]
        found.append(one)
    return site.Stack(fb, found, e.X, e.var, e.ls, s, a=a)


def find_sites_batched(kind, lik_kind, X, Y, M, var, ls, rule, starts, tols, max_sweeps, dampings, fb=None):
    """ep.find_sites for B models in lock step -> [_Sites] (module docstring).  X [n, d] shared or [B, n, d]; Y [n] shared or
    [B, n]; M = mean_function(X) [B, n]; var [B]; ls [B, nls]; rule: (nodes, weights) of the logit link, the group's; starts: per
    model the (tau, nu) to start at or None (zeros); tols, max_sweeps, dampings: per model ep_tol, max_sweeps and damping; fb: a
    FactorBatch(B, n, 1) to reuse."""
    return _sites(kind, lik_kind, X, Y, M, var, ls, rule, starts, tols, max_sweeps, dampings, fb).states


def search(ms, kind, lik_kind, X, Y, M, var, ls, starts, fb=None):
    """the search of a group of EPGP models ms, each with its own ep_tol, max_sweeps and damping, under the group's rule -> site.Stack"""
    return _sites(kind, lik_kind, X, Y, M, var, ls, ms[0]._rule(X.device), starts, [m.ep_tol for m in ms], [m.max_sweeps for m in ms],
                  [m.damping for m in ms], fb)


def _stack_gradients(kind, st, fb):
    """the closed form of EPEvidence.backward for the models of one Stack, in lock step -> (g [B, 1 + nls], None: there is no u)"""
    binv, ld, stride = _binv(fb, len(st.states))
    zero = torch.zeros_like(st.a)
    return _ops.laplace_grad_batched(kind, st.X, st.var, st.ls, st.s, binv, ld, stride, st.a, zero, zero), None


class BatchedEPEvidence(site.BatchedEvidence):
    """EPEvidence for B equal-shape models in LOCK STEP: find_sites_batched in the forward -> log Z_EP [B]; the closed form of
    EPEvidence.backward over the group in the backward (B^-1 by gpn_lml_kinv_batched, one batched gradient sweep with u = d1 = 0).
    The gradient for a model's m is a; afterwards every owner's _sites and ep_stats are what its own evaluation would have left."""
    family = site.GroupEvidence(search, lambda st: torch.stack([one.evidence for one in st.states]), _stack_gradients,
                                ep.EPEvidence.family.mean_gradient, STATS)


NODE = BatchedEPEvidence
