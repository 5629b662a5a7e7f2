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
A model that does not converge within its max_newton_iter, or whose factorisation reports info != 0, is replayed alone through
find_mode, which raises what it raises today: the whole call raises (models/_site_lockstep.py, which holds the scaffold this search
shares with EPGP's, says why a group is never mixed).

Out of scope: ragged (unequal-N) groups, composite kernels, dy > 1, Student-t, hipGraph capture, DistGPR.
"""
import torch

from .. import _native, _ops
from .._ops import _ptr, _stream
from . import _site_lockstep as site
from . import laplace
from ._lockstep import three_padded_matrices_bytes
from ._site_lockstep import _binv, _dots
from .laplace import MAX_HALVINGS, PSI_SLACK, W_FLOOR, LaplaceGP

# counters for tests and tools/laplace_lockstep_bench.py: lock-step searches, Newton rounds, host reads of trial rounds, and
# factorisations counted per MODEL (a round over k models adds k)
STATS = {"searches": 0, "rounds": 0, "trial_reads": 0, "factorisations": 0}

MAX_N = 8192        # the largest size measured (LAB 20: lock step 1.4-1.5 x the sequential rate there, 13-18 x at 512); beyond it a
#                     model is bound by its own factorisations and nothing is measured: such models stay sequential
MODEL = LaplaceGP   # the class whose models these groups take


def supported(n):
    """sizes whose LaplaceGP models are grouped: every measured shape is faster in lock step, none beyond MAX_N is measured"""
    return 1 <= int(n) <= MAX_N


def per_model_bytes(n, nls=1):
    """three padded N x N matrices per model (the factor slot + the backward's two), as for a GPR model, whatever nls"""
    return three_padded_matrices_bytes(n)


def _modes(kind, lik_kind, X, Y, M, var, ls, starts, tols, max_iters, fb=None):
    """find_modes -> the site.Stack of the B modes, with the [B, n] rows a, Ka, d1, d3 and the [B] rows value, sum_log_diag"""
    everyone, fb, work = site.begin(X, Y, M, var, ls, fb)
    B, n, dev = len(everyone.act), X.shape[-2], X.device
    STATS["searches"] += 1

    def alone(b):
        """model b has failed: its own sequential search raises what the model alone raises"""
        e = everyone
        laplace.find_mode(kind, lik_kind, e.X if e.X.dim() == 2 else e.X[b], e.Y if e.Y.dim() == 1 else e.Y[b], e.M[b], e.var[b:b + 1],
                          e.ls[b], a0=starts[b], newton_tol=tols[b], max_newton_iter=max_iters[b])
        raise site.disagreement("LaplaceGP", b)

    for b in range(B):
        if max_iters[b] <= 0:
            alone(b)                             # (raises RuntimeError: did not converge in 0 steps)
    run = everyone

    def kv(v):
        return _ops.laplace_matvec_batched(kind, run.X, run.var, run.ls, v, work=work)

    zero = torch.zeros(n, dtype=torch.float64, device=dev)
    warm = [start is not None for start in starts]
    if any(warm):
        a = torch.stack([start.detach().reshape(n) if start is not None else zero for start in starts])
        Ka = kv(a)
        if not all(warm):                        # a model without a start begins at a = 0, K a = 0 (no product)
            Ka = torch.where(torch.tensor(warm, device=dev)[:, None], Ka, zero)
    else:
        a = torch.zeros(B, n, dtype=torch.float64, device=dev)
        Ka = torch.zeros_like(a)
    f = run.M + Ka
    value, d1, W, _ = _ops.lik_derivs_batched(lik_kind, f, run.Y, want_d3=False)
    psi = value - 0.5 * _dots(a, Ka)
    final = [None] * B                           # per model its rows (a, Ka, f) at the mode
    steps, halvings = [0] * B, [0] * B
    while run.act:
        k = len(run.act)
        STATS["rounds"] += 1
        s = torch.sqrt(torch.clamp(W, min=W_FLOOR))
        b_ = W * Ka + d1
        site._factor_systems(kind, run.X, run.var, run.ls, s, fb, STATS, rhs=s * kv(b_))
        a_new = b_ - s * _ops.backsub_batched(fb, k)[:, 0]
        Ka_new = kv(a_new)
        t, accepted, h = [1.0] * k, [False] * k, 0
        while True:
            if all(tj == 1.0 for tj in t):
                a_t, Ka_t = a_new, Ka_new
            else:
                tt = torch.tensor(t, dtype=torch.float64, device=dev)[:, None]
                a_t = torch.where(tt == 1, a_new, a + tt * (a_new - a))
                Ka_t = torch.where(tt == 1, Ka_new, Ka + tt * (Ka_new - Ka))
            f_t = run.M + Ka_t
            value_t, d1_t, W_t, _ = _ops.lik_derivs_batched(lik_kind, f_t, run.Y, want_d3=False)
            psi_t = value_t - 0.5 * _dots(a_t, Ka_t)
            # the round's ONE host read: every model's psi before and after, its two maxima, its factorisation's info
            rows = torch.stack([psi_t, psi, (f_t - f).abs().amax(1), f_t.abs().amax(1), fb.info[:k].double()], 1).tolist()
            STATS["trial_reads"] += 1
            for j in range(k):
                if accepted[j]:
                    continue
                got, was, _max_df, _max_f, info = rows[j]
                if info != 0 or got >= was - PSI_SLACK * (1.0 + abs(was)) or h == MAX_HALVINGS:
                    accepted[j] = True           # (info != 0: nothing to halve, the model raises below)
                else:
                    t[j] *= 0.5
                    halvings[run.act[j]] += 1
            if all(accepted):
                break
            h += 1
        a, Ka, f, value, d1, W, psi = a_t, Ka_t, f_t, value_t, d1_t, W_t, psi_t
        keep = []
        for j, b in enumerate(run.act):
            _got, _was, max_df, max_f, info = rows[j]
            if info != 0:
                alone(b)                         # (raises NativeError: info != 0)
            steps[b] += 1
            if max_df <= tols[b] * (1.0 + max_f):
                final[b] = (a[j], Ka[j], f[j])
            elif steps[b] >= max_iters[b]:
                alone(b)                         # (raises RuntimeError: did not converge)
            else:
                keep.append(j)
        run, (a, Ka, f, value, d1, W, psi) = run.keep(keep, a, Ka, f, value, d1, W, psi)
    # the factor AT the mode, every model at once in its slot of the call
    a, Ka, F = (torch.stack([at_mode[i] for at_mode in final]) for i in range(3))
    value, d1, Wd, d3 = _ops.lik_derivs_batched(lik_kind, F, everyone.Y)
    s = torch.sqrt(torch.clamp(Wd, min=W_FLOOR))
    site._factor_systems(kind, everyone.X, everyone.var, everyone.ls, s, fb, STATS)
    sum_log_diag = site._sum_log_diags(fb, B).clone()       # (out of the shared buffers: the next call overwrites them)
    modes = []
    for b, info in enumerate(fb.info[:B].tolist()):
        if info != 0:
            alone(b)                             # (raises NativeError: the factorisation at the mode)
        mode = laplace._Mode()
        mode.a, mode.Ka, mode.f = a[b], Ka[b], F[b]
        mode.value, mode.d1, mode.W, mode.d3, mode.s = value[b], d1[b], Wd[b], d3[b], s[b]
        mode.factor, mode.generation, mode.sum_log_diag = fb.factor(b), fb.generation, sum_log_diag[b]
        mode.steps, mode.halvings = steps[b], halvings[b]
        modes.append(mode)
    return site.Stack(fb, modes, everyone.X, everyone.var, everyone.ls, s, a=a, Ka=Ka, d1=d1, d3=d3, value=value, sum_log_diag=sum_log_diag)


def find_modes(kind, lik_kind, X, Y, M, var, ls, starts, tols, max_iters, fb=None):
    """laplace.find_mode for B models in lock step -> [_Mode] (module docstring).  X [n, d] shared or [B, n, d]; Y [n] shared or
    [B, n]; M = mean_function(X) [B, n]; var [B]; ls [B, nls]; starts: per model the a to start at or None (a = 0); tols,
    max_iters: per model newton_tol and max_newton_iter; fb: a FactorBatch(B, n, 1) to reuse."""
    return _modes(kind, lik_kind, X, Y, M, var, ls, starts, tols, max_iters, fb).states


def search(ms, kind, lik_kind, X, Y, M, var, ls, starts, fb=None):
    """the search of a group of LaplaceGP models ms, each with its own newton_tol and max_newton_iter -> site.Stack"""
    return _modes(kind, lik_kind, X, Y, M, var, ls, starts, [m.newton_tol for m in ms], [m.max_newton_iter for m in ms], fb)


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
    """the closed form of LaplaceEvidence.backward for the models of one Stack, in lock step -> (g [B, 1 + nls], u [B, n])"""
    binv, ld, stride = _binv(fb, len(st.states))                         # B_b^-1 (lower triangle) at binv + 8 b stride
    sigma = _ops.laplace_diag_batched(kind, st.X, st.var, st.ls, st.s, binv, ld, stride)
    s2 = 0.5 * sigma * st.d3
    u = s2 - st.s * _solve_b_batched(fb, len(st.states), st.s * _ops.laplace_matvec_batched(kind, st.X, st.var, st.ls, s2))
    g = _ops.laplace_grad_batched(kind, st.X, st.var, st.ls, st.s, binv, ld, stride, st.a, u, st.d1)
    return g, u


class BatchedLaplaceEvidence(site.BatchedEvidence):
    """LaplaceEvidence for B equal-shape models in LOCK STEP: find_modes in the forward -> log q [B]; the closed form of
    LaplaceEvidence.backward over the group in the backward (B^-1 by gpn_lml_kinv_batched, one batched row-dot sweep, one batched
    product, the solve as gpn_trsm_right_lt_batched + gpn_backsub_batched, one batched gradient sweep).  The gradient for a model's
    m is d1 + u; afterwards every owner's _mode_a and newton_stats are what its own evaluation would have left."""
    family = site.GroupEvidence(search, lambda st: st.value - 0.5 * _dots(st.a, st.Ka) - st.sum_log_diag, _stack_gradients,
                                laplace.LaplaceEvidence.family.mean_gradient, STATS)


NODE = BatchedLaplaceEvidence
