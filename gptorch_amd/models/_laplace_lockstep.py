"""
LaplaceGP restarts and folds in LOCK STEP: the Newton mode search of models/laplace.py (find_mode), its evidence and its closed-form
gradients for B equal-shape models at once, every launch a strided-batch launch over the models (csrc/laplace.hip *_batched,
gpn_potrf_lower_batched, gpn_backsub_batched, gpn_lml_kinv_batched ...).  One evaluation of one model is 4-9 Newton steps of about
seven small launches and one host read per trial step; B restarts pay that B times, the group pays it once.

Every number a model receives is BIT-IDENTICAL to what its own log_likelihood() / loss().backward() / predict_f() computes:
  * per model the batched kernels run the single kernels' bodies on operands at a stride;
  * the elementwise torch expressions are find_mode's, on [B, n] stacks (a row's bits do not depend on the leading dimension);
  * every model has its own step length t_b and applies find_mode's acceptance rule to its own row of the ONE [B, 5] host read of a
    trial round (psi_t, psi, max |delta f|, max |f|, info); a model that has accepted waits (its trial is evaluated again at the
    same t_b: the same bits) while others halve;
  * a model that has converged leaves the search: the models still running are gathered (index_select) into a compact sub-batch
    that is factorised in the FIRST slots of the FactorBatch -- no kernel takes an index map, a converged model costs no further
    factorisation;
  * then one lock-step factorisation at every model's mode gives the factors and sum log L_ii.
A model that does not converge within its max_newton_iter, or whose factorisation reports info != 0, is dropped from the group and
replayed alone through find_mode, which raises what it raises today.

Out of scope: ragged (unequal-N) groups, composite kernels, dy > 1, Student-t, hipGraph capture, DistGPR.
"""
import ctypes

import torch

from .. import _native, _ops
from .._ops import _ptr, _stream
from . import laplace
from ._lockstep import three_padded_matrices_bytes
from .laplace import MAX_HALVINGS, PSI_SLACK, W_FLOOR

# counters for tests and tools/laplace_lockstep_bench.py: lock-step searches, Newton rounds, host reads of trial rounds, and
# factorisations counted per MODEL (a round over k models adds k)
STATS = {"searches": 0, "rounds": 0, "trial_reads": 0, "factorisations": 0}

MAX_N = 8192        # the largest size measured (LAB 20: lock step 1.4-1.5 x the sequential rate there, 13-18 x at 512); beyond it a
#                     model is bound by its own factorisations and nothing is measured: such models stay sequential


def supported(n):
    """sizes whose LaplaceGP models are grouped: every measured shape is faster in lock step, none beyond MAX_N is measured"""
    return 1 <= int(n) <= MAX_N


def per_model_bytes(n):
    """three padded N x N matrices per model (the factor slot + the backward's two), as for a GPR model"""
    return three_padded_matrices_bytes(n)


class _LockstepMode(laplace._Mode):
    """a _Mode whose factor is slot `slot` of the FactorBatch `fb`; `stack`: what the group's backward shares"""
    __slots__ = ("fb", "slot", "stack")


class _Stack:
    """the converged models of one find_modes call, stacked in slot order: ids (positions in the call), X, var, ls, y, and the
    [count, n] tensors a, Ka, d1, d3, s"""
    __slots__ = ("ids", "X", "var", "ls", "a", "Ka", "d1", "d3", "s", "value", "sum_log_diag", "generation")


def _dots(x, y):
    """<x_b, y_b> [k] of contiguous [k, n] stacks: laplace._dot's launch with the models on the batch dimension"""
    k, n = x.shape
    return _ops.dot2d_raw(_ptr(x), n, n, _ptr(y), n, n, 1, n, k, x.device)


def _potrf(fb, count, stats=None):
    fb.info[:count].zero_()
    st = _native.lib().gpn_potrf_lower_batched(_stream(fb.A.device), _ptr(fb.A), fb.n, fb.e, fb.ld, fb.sA, _ptr(fb.winv), fb.sW,
                                               _ptr(fb.info), count)
    _native.check(st, "gpn_potrf_lower_batched")
    (STATS if stats is None else stats)["factorisations"] += count


def _factor_systems(kind, X, var, ls, s, fb, rhs=None, stats=None):
    """laplace._factor_system for the first s.shape[0] slots of fb: B_b assembled and factorised, rhs [k, n] (None: zeros) forward-
    substituted on the way; nothing is read back.  stats: the counters that take the factorisations (None: this module's; EP's
    lock-step search, models/_ep_lockstep.py, hands in its own)."""
    k, n = s.shape
    _ops.laplace_system_batched(kind, X, var, ls, s, fb)
    extra = fb.A.view(fb.batch, fb.rows, fb.ld)[:k, n]
    if rhs is None:
        extra.zero_()
    else:
        extra[:, n:] = 0.0                       # the corner accumulates -alpha alpha^T (Factor.pack_rhs)
        extra[:, :n] = rhs
    _potrf(fb, k, stats)


def _sel(t, idx):
    return t.index_select(0, idx)


def _alone(kind, lik_kind, X, Y, M, var, ls, starts, tols, max_iters, b):
    """model b of the call through the sequential search (it raises what the model alone raises)"""
    return laplace.find_mode(kind, lik_kind, X if X.dim() == 2 else X[b], Y if Y.dim() == 1 else Y[b], M[b], var[b:b + 1], ls[b],
                             a0=starts[b], newton_tol=tols[b], max_newton_iter=max_iters[b])


def find_modes(kind, lik_kind, X, Y, M, var, ls, starts, tols, max_iters, fb=None):
    """laplace.find_mode for B models in lock step -> [_Mode] (module docstring).  X [n, d] shared or [B, n, d]; Y [n] shared or
    [B, n]; M = mean_function(X) [B, n]; var [B]; ls [B, nls]; starts: per model the a to start at or None (a = 0); tols,
    max_iters: per model newton_tol and max_newton_iter; fb: a FactorBatch(B, n, 1) to reuse."""
    B, n, dev = int(var.numel()), X.shape[-2], X.device
    var, ls, M = var.detach().reshape(B), ls.detach().reshape(B, -1), M.detach().reshape(B, n)
    X, Y = X.detach(), Y.detach()
    if fb is None or fb.batch != B or fb.n != n or fb.e != 1 or fb.A.device != dev:
        fb = _ops.FactorBatch(B, n, 1, dev)
    fb.generation += 1
    STATS["searches"] += 1
    work = _ops._rows_work(n, dev, None, B)
    modes = [None] * B

    def alone(b):
        modes[b] = _alone(kind, lik_kind, X, Y, M, var, ls, starts, tols, max_iters, b)

    act = list(range(B))
    for b in [b for b in act if max_iters[b] <= 0]:
        alone(b)
    act = [b for b in act if modes[b] is None]
    Xa, Ya, Ma, va, la = X, Y, M, var, ls
    if len(act) < B and act:
        idx = torch.tensor(act, device=dev)
        Xa, Ya = (_sel(X, idx) if X.dim() == 3 else X), (_sel(Y, idx) if Y.dim() == 2 else Y)
        Ma, va, la = _sel(M, idx), _sel(var, idx), _sel(ls, idx)

    def kv(v):
        return _ops.laplace_matvec_batched(kind, Xa, va, la, v, work=work)

    final = {}                                   # model -> its rows (a, Ka, f) at the mode
    steps, halvings = [0] * B, [0] * B
    if act:
        zero = torch.zeros(n, dtype=torch.float64, device=dev)
        warm = [starts[b] is not None for b in act]
        if any(warm):
            a = torch.stack([starts[b].detach().reshape(n) if starts[b] is not None else zero for b in act])
            Ka = kv(a)
            if not all(warm):                    # a model without a start begins at a = 0, K a = 0 (no product)
                Ka = torch.where(torch.tensor(warm, device=dev)[:, None], Ka, zero)
        else:
            a = torch.zeros(len(act), n, dtype=torch.float64, device=dev)
            Ka = torch.zeros_like(a)
        f = Ma + Ka
        value, d1, W, _ = _ops.lik_derivs_batched(lik_kind, f, Ya, want_d3=False)
        psi = value - 0.5 * _dots(a, Ka)
    while act:
        k = len(act)
        STATS["rounds"] += 1
        s = torch.sqrt(torch.clamp(W, min=W_FLOOR))
        b_ = W * Ka + d1
        _factor_systems(kind, Xa, va, la, s, fb, rhs=s * kv(b_))
        a_new = b_ - s * _ops.backsub_batched(fb, k)[:, 0]
        Ka_new = kv(a_new)
        t, accepted, failed, h = [1.0] * k, [False] * k, set(), 0
        while True:
            if all(tj == 1.0 for tj in t):
                a_t, Ka_t = a_new, Ka_new
            else:
                tt = torch.tensor(t, dtype=torch.float64, device=dev)[:, None]
                a_t = torch.where(tt == 1, a_new, a + tt * (a_new - a))
                Ka_t = torch.where(tt == 1, Ka_new, Ka + tt * (Ka_new - Ka))
            f_t = Ma + Ka_t
            value_t, d1_t, W_t, _ = _ops.lik_derivs_batched(lik_kind, f_t, Ya, want_d3=False)
            psi_t = value_t - 0.5 * _dots(a_t, Ka_t)
            # the round's ONE host read: every model's psi before and after, its two maxima, its factorisation's info
            rows = torch.stack([psi_t, psi, (f_t - f).abs().amax(1), f_t.abs().amax(1), fb.info[:k].double()], 1).tolist()
            STATS["trial_reads"] += 1
            for j in range(k):
                if accepted[j]:
                    continue
                got, was, _max_df, _max_f, info = rows[j]
                if info != 0:
                    failed.add(j)
                    accepted[j] = True
                elif got >= was - PSI_SLACK * (1.0 + abs(was)) or h == MAX_HALVINGS:
                    accepted[j] = True
                else:
                    t[j] *= 0.5
                    halvings[act[j]] += 1
            if all(accepted):
                break
            h += 1
        a, Ka, f, value, d1, W, psi = a_t, Ka_t, f_t, value_t, d1_t, W_t, psi_t
        keep = []
        for j, b in enumerate(act):
            if j in failed:
                alone(b)                         # (raises NativeError: info != 0)
                continue
            steps[b] += 1
            _got, _was, max_df, max_f, _info = rows[j]
            if max_df <= tols[b] * (1.0 + max_f):
                final[b] = (a[j], Ka[j], f[j])
            elif steps[b] >= max_iters[b]:
                alone(b)                         # (raises RuntimeError: did not converge)
            else:
                keep.append(j)
        if len(keep) < k:
            act = [act[j] for j in keep]
            if act:
                idx = torch.tensor(keep, device=dev)
                a, Ka, f, value, d1, W, psi = (_sel(v, idx) for v in (a, Ka, f, value, d1, W, psi))
                Xa, Ya = (_sel(Xa, idx) if Xa.dim() == 3 else Xa), (_sel(Ya, idx) if Ya.dim() == 2 else Ya)
                Ma, va, la = _sel(Ma, idx), _sel(va, idx), _sel(la, idx)
    ids = sorted(final)
    if not ids:
        return modes
    # the factor AT the mode, every converged model at once (slot = position in ids)
    st = _Stack()
    st.ids = ids
    if len(ids) == B:
        st.X, Yd, st.var, st.ls = X, Y, var, ls
    else:
        idx = torch.tensor(ids, device=dev)
        st.X, Yd = (_sel(X, idx) if X.dim() == 3 else X), (_sel(Y, idx) if Y.dim() == 2 else Y)
        st.var, st.ls = _sel(var, idx), _sel(ls, idx)
    st.a, st.Ka, F = (torch.stack([final[b][i] for b in ids]) for i in range(3))
    st.value, st.d1, Wd, st.d3 = _ops.lik_derivs_batched(lik_kind, F, Yd)
    st.s = torch.sqrt(torch.clamp(Wd, min=W_FLOOR))
    count = len(ids)
    _factor_systems(kind, st.X, st.var, st.ls, st.s, fb)
    lib = _native.lib()
    _native.check(lib.gpn_lml_reduce_batched(_stream(dev), _ptr(fb.A), n, 1, fb.ld, fb.sA, _ptr(fb.out), count), "gpn_lml_reduce_batched")
    st.sum_log_diag = fb.out[:count, 0].clone()  # (out of the shared buffers: the next call overwrites them)
    st.generation = fb.generation
    info = fb.info[:count].tolist()
    for slot, b in enumerate(ids):
        if info[slot] != 0:
            alone(b)                             # (raises NativeError: the factorisation at the mode)
            continue
        mode = _LockstepMode()
        mode.a, mode.Ka, mode.f = st.a[slot], st.Ka[slot], F[slot]
        mode.value, mode.d1, mode.W, mode.d3, mode.s = st.value[slot], st.d1[slot], Wd[slot], st.d3[slot], st.s[slot]
        mode.factor, mode.generation, mode.sum_log_diag = fb.factor(slot), fb.generation, st.sum_log_diag[slot]
        mode.steps, mode.halvings = steps[b], halvings[b]
        mode.fb, mode.slot, mode.stack = fb, slot, st
        modes[b] = mode
    return modes


def _solve_b_batched(fb, count, w):
    """laplace._solve_b for the first `count` slots: B_b^-1 w_b [count, n]"""
    n = fb.n
    rp = _ops.round_up(1, _ops.LEAF)
    rows = _ops.zeros(count * rp, fb.ld, fb.A.device).view(count, rp, fb.ld)
    rows[:, 0, :n] = w
    st = _native.lib().gpn_trsm_right_lt_batched(_stream(fb.A.device), _ptr(fb.A), n, fb.ld, fb.sA, _ptr(fb.winv), fb.sW, _ptr(rows), 1, fb.ld,
                                                 rp * fb.ld, count)
    _native.check(st, "gpn_trsm_right_lt_batched")
    fb.A.view(fb.batch, fb.rows, fb.ld)[:count, n, :n] = rows[:, 0, :n]
    return _ops.backsub_batched(fb, count)[:, 0]


def _stack_gradients(kind, st, fb):
    """the closed form of LaplaceEvidence.backward for the models of one _Stack, in lock step -> (g [count, 1 + nls], u [count, n])"""
    count, n = st.a.shape
    dev = st.a.device
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
    binv = wk.data_ptr() + 8 * koff                                      # B_b^-1 (lower triangle) at binv + 8 b stride
    sigma = _ops.laplace_diag_batched(kind, st.X, st.var, st.ls, st.s, binv, ld, stride)
    s2 = 0.5 * sigma * st.d3
    u = s2 - st.s * _solve_b_batched(fb, count, st.s * _ops.laplace_matvec_batched(kind, st.X, st.var, st.ls, s2))
    g = _ops.laplace_grad_batched(kind, st.X, st.var, st.ls, st.s, binv, ld, stride, st.a, u, st.d1)
    return g, u


class BatchedLaplaceEvidence(torch.autograd.Function):
    """LaplaceEvidence for B equal-shape models in LOCK STEP: find_modes in the forward -> log q [B]; the closed form of
    LaplaceEvidence.backward over the group in the backward (B^-1 by gpn_lml_kinv_batched, one batched row-dot sweep, one batched
    product, the solve as gpn_trsm_right_lt_batched + gpn_backsub_batched, one batched gradient sweep).  Inputs: X [n, d] shared or
    [B, n, d], Y [n, 1] shared or [B, n, 1], the CONSTRAINED variance [B] and length-scales [B, nls], owners (the models), a
    holder dict for the shared buffers, then every model's m = mean_function(X) [n, 1]; gradients for every m (d1 + u), variance
    and length-scales.  Afterwards every owner's _mode_a and newton_stats are what its own evaluation would have left; no owner's
    private factor cache points at the shared buffers."""

    @staticmethod
    def forward(ctx, X, Y, variance, length_scales, kind, lik_kind, owners, holder, *ms):
        B, n = len(owners), X.shape[-2]
        M = torch.stack([m.detach().reshape(n) for m in ms])
        y = Y.detach().reshape(n) if Y.dim() == 2 else Y.detach().reshape(B, n)
        var, ls = variance.detach().reshape(B), length_scales.detach().reshape(B, -1)
        modes = find_modes(kind, lik_kind, X, y, M, var, ls, [o._start(n) for o in owners], [o.newton_tol for o in owners],
                           [o.max_newton_iter for o in owners], fb=holder.get("fb"))
        stack = next((m.stack for m in modes if isinstance(m, _LockstepMode)), None)
        out = torch.empty(B, dtype=torch.float64, device=X.device)
        if stack is not None:
            holder["fb"] = next(m.fb for m in modes if isinstance(m, _LockstepMode))
            vals = stack.value - 0.5 * _dots(stack.a, stack.Ka) - stack.sum_log_diag
            if len(stack.ids) == B:
                out = vals
            else:
                out[torch.tensor(stack.ids, device=X.device)] = vals
        for b, (o, mode) in enumerate(zip(owners, modes)):
            if not isinstance(mode, _LockstepMode):                      # replayed alone: the sequential node's expression
                out[b] = (mode.value - 0.5 * laplace._dot(mode.a, mode.Ka) - mode.sum_log_diag).reshape(())
            o._remember(mode)
        ctx.kind, ctx.modes, ctx.stack = kind, modes, stack
        ctx.save_for_backward(X, variance, length_scales)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        X, variance, length_scales = ctx.saved_tensors
        kind, modes, st = ctx.kind, ctx.modes, ctx.stack
        B, n = len(modes), X.shape[-2]
        var, ls = variance.detach().reshape(B), length_scales.detach().reshape(B, -1)
        nls = ls.shape[1]
        g = torch.empty(B, 1 + nls, dtype=torch.float64, device=X.device)
        us = [None] * B
        if st is not None:
            fb = next(m.fb for m in modes if isinstance(m, _LockstepMode))
            if fb.generation != st.generation:
                # the shared buffers were refactorised by a later forward: rebuild this node's factors privately
                fb = _ops.FactorBatch(len(st.ids), n, 1, X.device)
                _factor_systems(kind, st.X, st.var, st.ls, st.s, fb)
            gs, u = _stack_gradients(kind, st, fb)
            if len(st.ids) == B:
                g = gs
            else:
                g[torch.tensor(st.ids, device=X.device)] = gs
            for slot, b in enumerate(st.ids):
                us[b] = u[slot]
        for b, mode in enumerate(modes):
            if not isinstance(mode, _LockstepMode):
                Xb = X if X.dim() == 2 else X[b]
                g[b], us[b] = laplace._evidence_gradients(kind, Xb, var[b:b + 1], ls[b], mode)
        go = grad_out.reshape(B)
        g_ms = tuple((go[b] * (modes[b].d1 + us[b])).reshape(n, 1) if ctx.needs_input_grad[8 + b] else None for b in range(B))
        return (None, None, (go * g[:, 0]).reshape(variance.shape), (go[:, None] * g[:, 1:1 + nls]).reshape(length_scales.shape),
                None, None, None, None) + g_ms
