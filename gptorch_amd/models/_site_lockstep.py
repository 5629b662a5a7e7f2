"""
What the lock-step searches of LaplaceGP (models/_laplace_lockstep.py) and EPGP (models/_ep_lockstep.py) share on the host -- the
groups of _lockstep.SiteKey: the batched factorisation and inversion helpers, the running sub-batch of the models still searching,
the stack a finished search leaves, and the ONE autograd node over it.  A family hands in its search, its value, its gradients and
its counters (Evidence); nothing here asks which family is calling.

A group is never mixed: every model of a search that returns has finished it in lock step, in its slot of the call.  A model that
fails (a search length of zero, a refused damping, info != 0, no convergence, a failed factorisation at the end) is replayed through
its own sequential search, which -- bit-identical per model -- fails in the same way and raises what the model alone raises; the
whole call raises and nobody's state has moved.  Should the replay RETURN, the two searches disagree: that is an error
(disagreement), not a state to continue from.
"""
import ctypes
from typing import Callable, NamedTuple

import torch

from .. import _native, _ops
from .._native import NativeError
from .._ops import _ptr, _stream


def _dots(x, y):
    """<x_b, y_b> [k] of contiguous [k, n] stacks: laplace._dot's launch with the models on the batch dimension"""
    k, n = x.shape
    return _ops.dot2d_raw(_ptr(x), n, n, _ptr(y), n, n, 1, n, k, x.device)


def _potrf(fb, count, stats):
    fb.info[:count].zero_()
    st = _native.lib().gpn_potrf_lower_batched(_stream(fb.A.device), _ptr(fb.A), fb.n, fb.e, fb.ld, fb.sA, _ptr(fb.winv), fb.sW,
                                               _ptr(fb.info), count)
    _native.check(st, "gpn_potrf_lower_batched")
    stats["factorisations"] += count


def _factor_systems(kind, X, var, ls, s, fb, stats, rhs=None):
    """laplace._factor_system for the first s.shape[0] slots of fb: B_b assembled and factorised, rhs [k, n] (None: zeros) forward-
    substituted on the way; nothing is read back.  stats: the calling family's counters, which take the factorisations."""
    k, n = s.shape
    _ops.laplace_system_batched(kind, X, var, ls, s, fb)
    extra = fb.A.view(fb.batch, fb.rows, fb.ld)[:k, n]
    if rhs is None:
        extra.zero_()
    else:
        extra[:, n:] = 0.0                       # the corner accumulates -alpha alpha^T (Factor.pack_rhs)
        extra[:, :n] = rhs
    _potrf(fb, k, stats)


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


def _sum_log_diags(fb, count):
    """sum log L_ii [count] of the factors in the first slots: a view of fb's buffers, which the next call overwrites"""
    st = _native.lib().gpn_lml_reduce_batched(_stream(fb.A.device), _ptr(fb.A), fb.n, 1, fb.ld, fb.sA, _ptr(fb.out), count)
    _native.check(st, "gpn_lml_reduce_batched")
    return fb.out[:count, 0]


def _sel(t, idx):
    return t.index_select(0, idx)


class SubBatch:
    """the models of a call that are still searching, compact in the first slots: act (their positions in the call, ascending) and
    their constants X [n, d] shared or [k, n, d], Y [n] shared or [k, n], M [k, n], var [k], ls [k, nls]"""

    def __init__(self, X, Y, M, var, ls, act):
        self.X, self.Y, self.M, self.var, self.ls, self.act = X, Y, M, var, ls, act

    def keep(self, slots, *rows):
        """-> (the SubBatch of the models at `slots`, ascending positions in this one; their rows of the [k, ...] tensors `rows`).
        Nobody has left, or nobody is left: no launch.  Otherwise ONE index_select per stacked tensor -- a shared X or Y is handed
        on as it is: no kernel takes an index map, the models still running move up into the first slots."""
        act = [self.act[j] for j in slots]
        if len(act) in (0, len(self.act)):
            return SubBatch(self.X, self.Y, self.M, self.var, self.ls, act), rows
        idx = torch.tensor(slots, device=self.M.device)
        rows = tuple(_sel(t, idx) for t in rows)
        X, Y = (_sel(self.X, idx) if self.X.dim() == 3 else self.X), (_sel(self.Y, idx) if self.Y.dim() == 2 else self.Y)
        return SubBatch(X, Y, _sel(self.M, idx), _sel(self.var, idx), _sel(self.ls, idx), act), rows


def begin(X, Y, M, var, ls, fb):
    """the start of a search over the B = var.numel() models of a call -> (the SubBatch of all of them, detached; the FactorBatch:
    fb where it fits the call, its generation moved on; the row kernels' workspace)"""
    B, n, dev = int(var.numel()), X.shape[-2], X.device
    everyone = SubBatch(X.detach(), Y.detach(), M.detach().reshape(B, n), var.detach().reshape(B), ls.detach().reshape(B, -1),
                        list(range(B)))
    if fb is None or fb.batch != B or fb.n != n or fb.e != 1 or fb.A.device != dev:
        fb = _ops.FactorBatch(B, n, 1, dev)
    fb.generation += 1
    return everyone, fb, _ops._rows_work(n, dev, None, B)


def disagreement(model, b):
    """what a search raises when the sequential replay of its failing model b returns (module docstring)"""
    return NativeError("%s: model %d of a lock-step group failed its search and its own sequential search did not -- the two "
                       "disagree, where they are bit-identical per model" % (model, b))


class Stack:
    """the B models of one finished search in slot order, which is their order in the call: states (every model's own, rows of the
    stacks), fb and its generation when it held their factors, what rebuilds those (X, var, ls, s [B, n]), a [B, n], and what
    LaplaceGP's value and gradients read beside it: Ka, d1, d3 [B, n], value, sum_log_diag [B] (EPGP: None)"""

    def __init__(self, fb, states, X, var, ls, s, a, Ka=None, d1=None, d3=None, value=None, sum_log_diag=None):
        self.fb, self.generation, self.states = fb, fb.generation, states
        self.X, self.var, self.ls, self.s, self.a = X, var, ls, s, a
        self.Ka, self.d1, self.d3, self.value, self.sum_log_diag = Ka, d1, d3, value, sum_log_diag


class Evidence(NamedTuple):
    """what the sequential node (laplace.SearchEvidence) asks of its family"""
    value: Callable            # state -> the evidence, 0-dim
    gradients: Callable        # (kind, X, var, ls, state) -> (g [1 + nls], u [n] or None)
    mean_gradient: Callable    # (state, u) -> d evidence / d m [n]


class GroupEvidence(NamedTuple):
    """what the lock-step node (BatchedEvidence) asks of its family"""
    search: Callable           # (owners, kind, lik_kind, X, Y, M, var, ls, starts, fb=) -> Stack
    value: Callable            # Stack -> the evidences [B]
    gradients: Callable        # (kind, Stack, fb) -> (g [B, 1 + nls], u [B, n] or None)
    mean_gradient: Callable    # (a model's state, its row of u) -> d evidence / d m [n]: the sequential family's
    stats: dict                # the counters that take a private rebuild's factorisations


class BatchedEvidence(torch.autograd.Function):
    """the lock-step evidence of a group as ONE autograd node; a family's node is a subclass that sets `family` (a GroupEvidence;
    forward and backward, static methods, find it through ctx._forward_cls: the class whose apply() was called, which
    torch.autograd sets on every node's class).
    Inputs: X [n, d] shared or [B, n, d], Y [n, 1] shared or [B, n, 1], the CONSTRAINED variance [B] and length-scales [B, nls], the
    kernel and likelihood kinds, owners (the models), a holder dict for the shared buffers, then every model's
    m = mean_function(X) [n, 1]; gradients for every m, variance and length-scales.  Afterwards every owner remembers what its own
    evaluation would have left; no owner's private factor cache points at the shared buffers."""
    family = None

    @staticmethod
    def forward(ctx, X, Y, variance, length_scales, kind, lik_kind, owners, holder, *ms):
        family = ctx._forward_cls.family
        B, n = len(owners), X.shape[-2]
        M = torch.stack([m.detach().reshape(n) for m in ms])
        y = Y.detach().reshape(n) if Y.dim() == 2 else Y.detach().reshape(B, n)
        var, ls = variance.detach().reshape(B), length_scales.detach().reshape(B, -1)
        st = family.search(owners, kind, lik_kind, X, y, M, var, ls, [o._start(n) for o in owners], fb=holder.get("fb"))
        holder["fb"] = st.fb
        for o, state in zip(owners, st.states):
            o._remember(state)
        ctx.kind, ctx.stack = kind, st
        ctx.save_for_backward(X, variance, length_scales)
        return family.value(st)

    @staticmethod
    def backward(ctx, grad_out):
        family = ctx._forward_cls.family
        X, variance, length_scales = ctx.saved_tensors
        kind, st = ctx.kind, ctx.stack
        B, n, nls = len(st.states), X.shape[-2], st.ls.shape[1]
        fb = st.fb
        if fb.generation != st.generation:
            # the shared buffers were refactorised by a later forward: rebuild this node's factors privately
            fb = _ops.FactorBatch(B, n, 1, X.device)
            _factor_systems(kind, st.X, st.var, st.ls, st.s, fb, family.stats)
        g, u = family.gradients(kind, st, fb)
        go = grad_out.reshape(B)
        g_ms = tuple((go[b] * family.mean_gradient(st.states[b], None if u is None else u[b])).reshape(n, 1)
                     if ctx.needs_input_grad[8 + b] else None for b in range(B))
        return (None, None, (go * g[:, 0]).reshape(variance.shape), (go[:, None] * g[:, 1:1 + nls]).reshape(length_scales.shape),
                None, None, None, None) + g_ms
