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
  * then ONE lock-step posterior at every finished model's sites, the moments without an update and sum log L_ii give the factors,
    the cavity moments and the evidence: all of the same (tau, nu), as find_sites leaves them.
A model whose factorisation reports info != 0, or that exhausts its max_sweeps, is dropped from the group and replayed alone through
find_sites, which raises what it raises today.

Out of scope: ragged (unequal-N) groups, composite kernels, dy > 1, Poisson and Student-t, sequential (rank-one) EP, hipGraph capture,
DistGPR.
"""
import ctypes

import torch

from .. import _native, _ops
from .._ops import _ptr, _stream
from . import ep
from ._laplace_lockstep import _dots, _factor_systems, _sel
from .ep import STALL_BELOW
from .laplace import W_FLOOR

# counters for tests and tools/ep_lockstep_bench.py: lock-step searches, sweeps, host reads, and factorisations counted per MODEL
# (a sweep over k models adds k)
STATS = {"searches": 0, "sweeps": 0, "reads": 0, "factorisations": 0}

MAX_N = 8192        # the largest size measured (LAB 23, profiles/ep_lockstep.json): the lock-step median is below the sequential one in
#                     the cold and the warm column of every measured shape up to it; beyond it nothing is measured: sequential


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


class _LockstepSites(ep._Sites):
    """a _Sites whose factor is a slot of the FactorBatch `fb`; `stack`: what the group's backward shares"""
    __slots__ = ("fb", "stack")


class _Stack:
    """the finished models of one find_sites_batched call, stacked in slot order: ids (positions in the call), X, var, ls and the
    [count, n] tensors a, s"""
    __slots__ = ("ids", "X", "var", "ls", "a", "s", "generation")


def _binv(fb, count):
    """B_b^-1 (lower triangles) of the first `count` factorised slots -> (device address of model 0's, leading dimension, doubles
    from one model's to the next); in fb's workspace, valid until the next call"""
    n, dev = fb.n, fb.A.device
    lib = _native.lib()
    lay = (ctypes.c_int64 * 4)()
    _native.check(lib.gpn_lml_kinv_layout(n, 1, lay), "gpn_lml_kinv_layout")
    ld, koff, _aoff, stride = (int(v) for v in lay)
    need = max(1, int(lib.gpn_lml_kinv_batched_work_bytes(n, 1, count)) // 8)
    if fb._backward_work is None or fb._backward_work.numel() < need:
        fb._backward_work = torch.empty(need, dtype=torch.float64, device=dev)
    wk = fb._backward_work
    _native.check(lib.gpn_lml_kinv_batched(_stream(dev), count, n, _ptr(fb.A), fb.ld, fb.sA, _ptr(fb.winv), fb.sW, 1, _ptr(wk)),
                  "gpn_lml_kinv_batched")
    return wk.data_ptr() + 8 * koff, ld, stride


def _posteriors(kind, X, M, var, ls, tau, nu, fb, work):
    """ep._posterior for the k = tau.shape[0] models in the first slots of fb -> (s, a, K a, mu, sigma2), each [k, n]; the slots
    hold the factors afterwards."""
    k = tau.shape[0]
    s = torch.sqrt(torch.clamp(tau, min=W_FLOOR))
    w = nu - tau * M
    _factor_systems(kind, X, var, ls, s, fb, rhs=s * _ops.laplace_matvec_batched(kind, X, var, ls, w, work=work), stats=STATS)
    a = w - s * _ops.backsub_batched(fb, k)[:, 0]
    Ka = _ops.laplace_matvec_batched(kind, X, var, ls, a, work=work)
    binv, ld, stride = _binv(fb, k)
    sigma2 = _ops.laplace_diag_batched(kind, X, var, ls, s, binv, ld, stride, work=work)
    return s, a, Ka, M + Ka, sigma2


def find_sites_batched(kind, lik_kind, X, Y, M, var, ls, rule, starts, tols, max_sweeps, dampings, fb=None):
    """ep.find_sites for B models in lock step -> [_Sites] (module docstring).  X [n, d] shared or [B, n, d]; Y [n] shared or
    [B, n]; M = mean_function(X) [B, n]; var [B]; ls [B, nls]; rule: (nodes, weights) of the logit link, the group's; starts: per
    model the (tau, nu) to start at or None (zeros); tols, max_sweeps, dampings: per model ep_tol, max_sweeps and damping; fb: a
    FactorBatch(B, n, 1) to reuse."""
    B, n, dev = int(var.numel()), X.shape[-2], X.device
    var, ls, M = var.detach().reshape(B), ls.detach().reshape(B, -1), M.detach().reshape(B, n)
    X, Y = X.detach(), Y.detach()
    if fb is None or fb.batch != B or fb.n != n or fb.e != 1 or fb.A.device != dev:
        fb = _ops.FactorBatch(B, n, 1, dev)
    fb.generation += 1
    STATS["searches"] += 1
    work = _ops._rows_work(n, dev, None, B)
    sites = [None] * B

    def alone(b):
        # model b of the call through the sequential search (it raises what the model alone raises)
        sites[b] = ep.find_sites(kind, lik_kind, X if X.dim() == 2 else X[b], Y if Y.dim() == 1 else Y[b], M[b], var[b:b + 1], ls[b],
                                 rule=rule, sites0=starts[b], ep_tol=tols[b], max_sweeps=max_sweeps[b], damping=dampings[b])

    for b in range(B):
        # (the dampings travel as a device array that gpn_ep_sites_batched cannot check: a bad one meets gpn_ep_sites' own refusal)
        if max_sweeps[b] <= 0 or not 0.0 < float(dampings[b]) <= 1.0:
            alone(b)
    act = [b for b in range(B) if sites[b] is None]
    rho_all = torch.tensor([float(r) for r in dampings], dtype=torch.float64, device=dev)
    Xa, Ya, Ma, va, la, rho = X, Y, M, var, ls, rho_all
    if act:
        zero = torch.zeros(n, dtype=torch.float64, device=dev)
        tau = torch.stack([zero if starts[b] is None else starts[b][0].detach().reshape(n) for b in act])
        nu = torch.stack([zero if starts[b] is None else starts[b][1].detach().reshape(n) for b in act])
        if len(act) < B:
            idx = torch.tensor(act, device=dev)
            Xa, Ya = (_sel(X, idx) if X.dim() == 3 else X), (_sel(Y, idx) if Y.dim() == 2 else Y)
            Ma, va, la, rho = _sel(M, idx), _sel(var, idx), _sel(ls, idx), _sel(rho_all, idx)
    final = {}                                   # model -> (its rows tau, nu at the sites found, stalled)
    sweeps, before = [0] * B, [[] for _ in range(B)]
    while act:
        k = len(act)
        STATS["sweeps"] += 1
        _, _, _, mu, sigma2 = _posteriors(kind, Xa, Ma, va, la, tau, nu, fb, work)
        tau, nu, _, _, _, stats = _ops.ep_sites_batched(lik_kind, Ya, Ma, mu, sigma2, tau, nu, rho, *rule, want_moments=False)
        # the sweep's ONE host read: every model's statistics and its factorisation's info word
        rows = torch.cat([stats, fb.info[:k].double()[:, None]], 1).tolist()
        STATS["reads"] += 1
        keep = []
        for j, b in enumerate(act):
            _, _, dtau, dnu, mtau, mnu, info = rows[j]
            sweeps[b] += 1
            if info != 0:
                alone(b)                         # (raises NativeError: info != 0)
                continue
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
        if len(keep) < k:
            act = [act[j] for j in keep]
            if act:
                idx = torch.tensor(keep, device=dev)
                tau, nu, rho = _sel(tau, idx), _sel(nu, idx), _sel(rho, idx)
                Xa, Ya = (_sel(Xa, idx) if Xa.dim() == 3 else Xa), (_sel(Ya, idx) if Ya.dim() == 2 else Ya)
                Ma, va, la = _sel(Ma, idx), _sel(va, idx), _sel(la, idx)
    ids = sorted(final)
    if not ids:
        return sites
    # the posterior, the moments and the factor AT the sites, every finished model at once (slot = position in ids)
    st = _Stack()
    st.ids = ids
    count = len(ids)
    if count == B:
        st.X, Yd, Md, st.var, st.ls, rho = X, Y, M, var, ls, rho_all
    else:
        idx = torch.tensor(ids, device=dev)
        st.X, Yd = (_sel(X, idx) if X.dim() == 3 else X), (_sel(Y, idx) if Y.dim() == 2 else Y)
        Md, st.var, st.ls, rho = _sel(M, idx), _sel(var, idx), _sel(ls, idx), _sel(rho_all, idx)
    tau, nu = (torch.stack([final[b][i] for b in ids]) for i in range(2))
    st.s, st.a, Ka, mu, sigma2 = _posteriors(kind, st.X, Md, st.var, st.ls, tau, nu, fb, work)
    _, _, _, mu_hat, s2_hat, stats = _ops.ep_sites_batched(lik_kind, Yd, Md, mu, sigma2, tau, nu, rho, *rule, moments_only=True)
    _native.check(_native.lib().gpn_lml_reduce_batched(_stream(dev), _ptr(fb.A), n, 1, fb.ld, fb.sA, _ptr(fb.out), count),
                  "gpn_lml_reduce_batched")
    evidence = stats[:, 1] + 0.5 * _dots(nu - tau * Md, Ka) - fb.out[:count, 0]
    st.generation = fb.generation
    info = fb.info[:count].tolist()
    for slot, b in enumerate(ids):
        if info[slot] != 0:
            alone(b)                             # (raises NativeError: the factorisation at the converged sites)
            continue
        one = _LockstepSites()
        one.tau, one.nu, one.a, one.Ka, one.s = tau[slot], nu[slot], st.a[slot], Ka[slot], st.s[slot]
        one.mu, one.sigma2, one.mu_hat, one.s2_hat = mu[slot], sigma2[slot], mu_hat[slot], s2_hat[slot]
        one.factor, one.generation, one.evidence = fb.factor(slot), fb.generation, evidence[slot]
        one.sweeps, one.stalled = sweeps[b], final[b][2]
        one.fb, one.stack = fb, st
        sites[b] = one
    return sites


def _stack_gradients(kind, st, fb):
    """the closed form of EPEvidence.backward for the models of one _Stack, in lock step -> g [count, 1 + nls]"""
    binv, ld, stride = _binv(fb, len(st.ids))
    zero = torch.zeros_like(st.a)
    return _ops.laplace_grad_batched(kind, st.X, st.var, st.ls, st.s, binv, ld, stride, st.a, zero, zero)


class BatchedEPEvidence(torch.autograd.Function):
    """EPEvidence for B equal-shape models in LOCK STEP: find_sites_batched in the forward -> log Z_EP [B]; the closed form of
    EPEvidence.backward over the group in the backward (B^-1 by gpn_lml_kinv_batched, one batched gradient sweep with u = d1 = 0).
    Inputs: X [n, d] shared or [B, n, d], Y [n, 1] shared or [B, n, 1], the CONSTRAINED variance [B] and length-scales [B, nls], the
    kernel and likelihood kinds, owners (the models), a holder dict for the shared buffers, then every model's m = mean_function(X)
    [n, 1]; gradients for every m (a), variance and length-scales.  Afterwards every owner's _sites and ep_stats are what its own
    evaluation would have left; no owner's private factor cache points at the shared buffers."""

    @staticmethod
    def forward(ctx, X, Y, variance, length_scales, kind, lik_kind, owners, holder, *ms):
        B, n = len(owners), X.shape[-2]
        M = torch.stack([m.detach().reshape(n) for m in ms])
        y = Y.detach().reshape(n) if Y.dim() == 2 else Y.detach().reshape(B, n)
        var, ls = variance.detach().reshape(B), length_scales.detach().reshape(B, -1)
        sites = find_sites_batched(kind, lik_kind, X, y, M, var, ls, owners[0]._rule(X.device), [o._start(n) for o in owners],
                                   [o.ep_tol for o in owners], [o.max_sweeps for o in owners], [o.damping for o in owners],
                                   fb=holder.get("fb"))
        first = next((s for s in sites if isinstance(s, _LockstepSites)), None)
        if first is not None:
            holder["fb"] = first.fb
        for o, s in zip(owners, sites):
            o._remember(s)
        ctx.kind, ctx.sites, ctx.stack = kind, sites, None if first is None else first.stack
        ctx.save_for_backward(X, variance, length_scales)
        return torch.stack([s.evidence for s in sites])

    @staticmethod
    def backward(ctx, grad_out):
        X, variance, length_scales = ctx.saved_tensors
        kind, sites, st = ctx.kind, ctx.sites, ctx.stack
        B, n = len(sites), X.shape[-2]
        var, ls = variance.detach().reshape(B), length_scales.detach().reshape(B, -1)
        nls = ls.shape[1]
        g = torch.empty(B, 1 + nls, dtype=torch.float64, device=X.device)
        if st is not None:
            fb = next(s.fb for s in sites if isinstance(s, _LockstepSites))
            if fb.generation != st.generation:
                # the shared buffers were refactorised by a later forward: rebuild this node's factors privately
                fb = _ops.FactorBatch(len(st.ids), n, 1, X.device)
                _factor_systems(kind, st.X, st.var, st.ls, st.s, fb, stats=STATS)
            gs = _stack_gradients(kind, st, fb)
            if len(st.ids) == B:
                g = gs
            else:
                g[torch.tensor(st.ids, device=X.device)] = gs
        for b, s in enumerate(sites):
            if not isinstance(s, _LockstepSites):
                g[b] = ep._evidence_gradients(kind, X if X.dim() == 2 else X[b], var[b:b + 1], ls[b], s)
        go = grad_out.reshape(B)
        g_ms = tuple((go[b] * sites[b].a).reshape(n, 1) if ctx.needs_input_grad[8 + b] else None for b in range(B))
        return (None, None, (go * g[:, 0]).reshape(variance.shape), (go[:, None] * g[:, 1:1 + nls]).reshape(length_scales.shape),
                None, None, None, None) + g_ms
