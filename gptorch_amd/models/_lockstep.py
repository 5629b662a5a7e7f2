"""
Several INDEPENDENT models evaluated in lock step: which models can share a call (the group keys and their memory-capacity
rule), the buffers a group keeps between calls, and the public batched entry points batched_log_likelihood,
batched_loss_and_grad and batched_factorise.  (GPR and VFE are imported where they are needed: models/gpr.py imports this
module.)
"""
import collections
from typing import NamedTuple, Optional

import torch

from .. import _expr, _native, _ops, mean_functions


class GroupKey(NamedTuple):
    """what the GPR models of one stationary lock-step group have in common"""
    kind: str                         # kernels.Stationary._kind
    shape: tuple                      # X's (n, d); a ragged group: (rows of its largest model, d)
    dy: int
    nls: int                          # number of length scales (1 or d: ARD)
    device: torch.device
    sizes: Optional[tuple] = None     # a RAGGED group: every model's own number of rows
    objective: str = "lml"            # what the group's models fit (GPR.objective): "loo" groups run _ops.BatchedGPRLooLik


# Lock-step buffers reused between calls (a search calls batched_log_likelihood / batched_loss_and_grad once per optimiser
# step): keyed by the FULL group key + batch size -- two groups of one call can never share an entry (round-4 advice: keyed
# by (device, batch, n, dy) only, two groups of equal count / N / dy but different kernel kind or ARD shared one buffer and
# the first group read the second group's results) -- least recently used first out, bounded in entries and bytes;
# release_batch_buffers() drops them all.
_BATCH_BUFFERS = collections.OrderedDict()    # (group key, batch) -> holder dict {"fb": _ops.FactorBatch}
BATCH_BUFFER_MAX_ENTRIES = 4
BATCH_BUFFER_MAX_BYTES = 48 << 30


def _held_bytes():
    # (a leave-one-out group keeps its right-hand sides, Q and the sweep's partials beside its FactorBatch; the inversion's workspace
    #  is the FactorBatch's _backward_work)
    return sum(v["fb"].nbytes() for v in _BATCH_BUFFERS.values() if "fb" in v) + \
        sum(8 * v[name].numel() for v in _BATCH_BUFFERS.values() for name in _ops.LOO_HOLDER_BUFFERS if v.get(name) is not None)


def _batch_holder(key):
    h = _BATCH_BUFFERS.pop(key, None)
    if h is None:
        h = {}
    _BATCH_BUFFERS[key] = h                     # most recently used last
    while len(_BATCH_BUFFERS) > 1 and (len(_BATCH_BUFFERS) > BATCH_BUFFER_MAX_ENTRIES or _held_bytes() > BATCH_BUFFER_MAX_BYTES):
        _BATCH_BUFFERS.popitem(last=False)
    return h


def release_batch_buffers():
    """free the factor buffers batched_log_likelihood / batched_loss_and_grad keep between calls."""
    _BATCH_BUFFERS.clear()


def _shared_transform(params):
    t0 = params[0]._transform
    return t0 if all(p._transform == t0 for p in params) else None


def _stacked(params, differentiable=False):
    """constrained values of same-shaped Params as one [B, ...] tensor: one stack + ONE transform when they share it (differentiable:
    of the Params themselves -- StackBackward hands every Param its own gradient row --, else of their .data)."""
    t0 = _shared_transform(params)
    if t0 is None:
        return torch.stack([p.transform() for p in params])
    return t0(torch.stack(list(params) if differentiable else [p.data for p in params]))


def _group_param_lists(ms):
    return [m.kernel.variance for m in ms], [m.kernel.length_scales for m in ms], [m.likelihood.variance for m in ms]


def _group_hypers(ms, differentiable=False):
    """(variance [B], length scales [B, 1 or d], noise [B]) of a group of models over one stationary kernel each.
    Host side: a handful of launches per GROUP, none per model (a per-model exp / subtraction / comparison costs more than the
    model's share of the batch at N = 512)"""
    var, ls, nz = (_stacked(pl, differentiable) for pl in _group_param_lists(ms))
    return var.reshape(len(ms)), ls.reshape(len(ms), -1), nz.reshape(len(ms))


def _place_all(models):
    """settings.auto_device: CPU-constructed models move to the GPU (once) BEFORE they are grouped -- the grouping looks at
    m.X.is_cuda, and a model that is still on the CPU would silently fall out of every lock-step group."""
    for m in models:
        place = getattr(m, "_auto_place", None)
        if place is not None:
            place()


def _group_key(m):
    k = m._stationary()
    return GroupKey(k._kind, tuple(m.X.shape), m.Y.shape[1], int(k.length_scales.numel()), m.X.device)


RAGGED_MIN_FRACTION = 0.75      # a ragged group's smallest model has at least this fraction of its largest model's rows
RAGGED_POOL_BELOW = 8            # equal-size groups of fewer models than this may merge with neighbouring sizes into one ragged group
LOCKSTEP_MEMORY_FRACTION = 0.7   # of the device's free memory (+ what the lock-step cache already holds) a group may take


def _panel_regime(n):
    """models whose sizes select the same panel levels of the factorisation (gpn_potrf_panel_levels) -- and none of which is refined --
    can be padded into one ragged lock-step group; None: no ragged group for this size"""
    if n <= 2 * _ops.LEAF or n >= _ops.refine_min_n():
        return None
    return 0 if n <= 2048 else 1 if n < 20480 else 2


def _capacity(per_model, device, held=0):
    """how many models of per_model bytes each fit one lock-step call (held: bytes the call would take over rather than allocate)"""
    try:
        free, _total = torch.cuda.mem_get_info(device)
    except Exception:
        return 1 << 30
    return max(2, int(LOCKSTEP_MEMORY_FRACTION * (free + held)) // per_model)


def _stationary_capacity(n, device):
    """... for GPR models of n rows: 3 padded N x N matrices per model (factor + the backward's two); the buffer cache's factors count
    as free"""
    ld = -(-int(n) // 128) * 128 + 128
    return _capacity(3 * 8 * (ld + 16) * ld, device, held=_held_bytes())


def _chunks(key, g, cap):
    """a group split into chunks of at most cap models: [(key, indices)] (singletons fall to the sequential path)"""
    return [(key, g[at:at + cap]) for at in range(0, len(g), cap) if len(g[at:at + cap]) >= 2]


def _lockstep_groups(models, for_grad=False):
    """[(GroupKey, indices)] of the models that can share one lock-step call, grouped by (kernel kind, n, d, dy, ARD, device):
    GPR over a native stationary kernel.  for_grad (the stacked-parameter
    optimiser loop of multi_start_optimize): also no priors (loss() = -(LML + log prior), model.py:158-197, is formed per model).
    Models left alone by that (cross-validation folds of unequal length, learning curves) form RAGGED groups: same kind / d / dy / ARD,
    zero mean, different n within one panel regime, each padded to the group's largest model with identity rows
    (_ops.lml_forward_batched(n_of=...)); their key carries the sizes."""
    from .gpr import GPR
    groups = {}
    for i, m in enumerate(models):
        # GPR's own log_likelihood only: other GPModels (VFE), and subclasses that evaluate differently (DistGPR: collective, on the
        # process grid), take their own path
        if not isinstance(m, GPR) or type(m).log_likelihood is not GPR.log_likelihood:
            continue
        k = m._stationary()
        if k is None or not m.X.is_cuda or m.X.shape[0] == 0:
            continue
        if m.objective == "kfold":                                       # k-fold models run one by one, whatever is asked of them
            continue
        if for_grad and (_has_priors([m]) or m.objective != "lml"):      # (another objective: loss() is formed by the model itself)
            continue
        groups.setdefault(_group_key(m), []).append(i)
    out, pool = [], {}
    for key, g in groups.items():
        # Small equal-size groups and singletons of ragged-eligible models are POOLED: folds of n and n - 1 rows make one ragged group
        # of all of them rather than two small groups.  (Groups of RAGGED_POOL_BELOW models or more stay as they are -- multi-start
        # restarts on one data set share its tensors --, and so does everything the stacked optimiser loop asks for.)
        regime = _panel_regime(key.shape[0])
        if not for_grad and len(g) < RAGGED_POOL_BELOW and regime is not None and \
                all(type(models[i].mean_function) is mean_functions.Zero for i in g):
            pool.setdefault((key._replace(shape=key.shape[1:]), regime), []).extend(g)
            continue
        # a lock-step group holds B factor buffers AND (with gradients) a backward workspace of two more N x N matrices per model at
        # once: groups that would not fit the device's free memory are split into chunks that do
        out += _chunks(key, g, _stationary_capacity(key.shape[0], key.device))
    for (common, _regime), g in pool.items():
        g = sorted(g, key=lambda i: (-models[i].X.shape[0], i))
        at = 0
        while at < len(g):
            nmax = models[g[at]].X.shape[0]
            end = at + 1
            cap = _stationary_capacity(nmax, common.device)
            while end < len(g) and end - at < cap and models[g[end]].X.shape[0] >= RAGGED_MIN_FRACTION * nmax:
                end += 1
            if end - at >= 2:
                chunk = sorted(g[at:end])
                sizes = tuple(models[i].X.shape[0] for i in chunk)
                # (all of one size after all: the ordinary equal-size group)
                out.append((common._replace(shape=(nmax,) + common.shape, sizes=sizes if len(set(sizes)) > 1 else None), chunk))
            at = end
    return out


def _loo_groups(models):
    """[(GroupKey, indices)] of the GPR(objective="loo") models that can share one lock-step evaluation (_ops.BatchedGPRLooLik): GPR's
    own loss / loo_log_predictive over a native stationary kernel on the GPU, of a size _loo_lockstep.supported() admits, grouped by
    (kernel kind, X's shape, dy, ARD or not, device) -- equal shapes only, no ragged pooling -- and split into chunks that fit the
    device's free memory; singletons stay sequential.  The key's objective field is "loo": it selects the node and keeps the cached
    buffers apart from those of an LML group of the same shape."""
    from . import _loo_lockstep
    from .gpr import GPR
    groups = {}
    for i, m in enumerate(models):
        if not isinstance(m, GPR) or m.objective != "loo":
            continue
        if type(m).loss is not GPR.loss or type(m)._loss is not GPR._loss or type(m).loo_log_predictive is not GPR.loo_log_predictive:
            continue                                     # a subclass that evaluates differently takes its own path
        k = m._stationary()
        if k is None or not m.X.is_cuda or not _loo_lockstep.supported(m.X.shape[0]):
            continue
        groups.setdefault(_group_key(m)._replace(objective="loo"), []).append(i)
    out = []
    for key, g in groups.items():
        out += _chunks(key, g, _capacity(_loo_lockstep.per_model_bytes(key.shape[0], key.dy, key.nls), key.device, held=_held_bytes()))
    return out


def _expression_groups(models):
    """[(key, indices, programs)] of the GPR models over COMPOSITE kernels of one structure (equal _expr.Program.signature(),
    n, d, dy, device) that can share the kernel-independent launches of an evaluation (_expr.BatchedExprLogLik)."""
    from .gpr import GPR
    groups = {}
    for i, m in enumerate(models):
        if not isinstance(m, GPR) or type(m).log_likelihood is not GPR.log_likelihood or m._stationary() is not None:
            continue
        if not m.X.is_cuda or m.X.shape[0] == 0 or m.objective == "kfold":   # (k-fold models run one by one)
            continue
        prog = m._expression(m.X)
        if prog is None:
            continue
        key = ("expr", prog.signature(), tuple(m.X.shape), m.Y.shape[1], m.X.device)
        groups.setdefault(key, ([], []))
        groups[key][0].append(i)
        groups[key][1].append(prog)
    return [(key, g, progs) for key, (g, progs) in groups.items() if len(g) >= 2]


def _vfe_groups(models):
    """[(key, indices)] of the VFE models (sparse_gpr.py:108-153) that can share one lock-step evaluation
    (_vfe_lockstep.BatchedVFEBound): one native stationary kind, equal (N, D, dy, M, ARD), on one device, in the single-chunk regime
    (_vfe_lockstep.supported); split into chunks that fit the device's free memory.
    key = ("vfe", kind, X's shape, dy, number of length scales, Z's shape, device)."""
    from . import _vfe_lockstep
    from .sparse_gpr import VFE
    groups = {}
    for i, m in enumerate(models):
        if not isinstance(m, VFE) or type(m).log_likelihood is not VFE.log_likelihood or type(m)._bound is not VFE._bound:
            continue
        k = m._native_kernel()
        if k is None or not m.X.is_cuda or not _vfe_lockstep.supported(m.X.shape[0], m.Z.shape[0]):
            continue
        key = ("vfe", k._kind, tuple(m.X.shape), m.Y.shape[1], int(k.length_scales.numel()), tuple(m.Z.shape), m.X.device)
        groups.setdefault(key, []).append(i)
    out = []
    for key, g in groups.items():
        _tag, _kind, (n, _d), dy, _nls, (n_inducing, _dz), device = key
        out += _chunks(key, g, _capacity(_vfe_lockstep.per_model_bytes(n, n_inducing, dy), device))
    return out


def _vfe_group_bound(ms, key, differentiable):
    """the lock-step bounds [B] of one _vfe_groups group (autograd-connected to every model's Params when differentiable)"""
    from . import _vfe_lockstep
    m0 = ms[0]
    same_x = all(m.X.data_ptr() == m0.X.data_ptr() for m in ms)
    same_y = same_x and all(m.Y.data_ptr() == m0.Y.data_ptr() for m in ms)
    X = m0.X if same_x else torch.stack([m.X for m in ms])
    Y = m0.Y if same_y else torch.stack([m.Y for m in ms])               # sparse_gpr.py:125 quirk: err = Y (Zero mean only)
    var, ls, s2 = _group_hypers(ms, differentiable)
    Z = torch.stack([m.Z for m in ms]) if differentiable else torch.stack([m.Z.data for m in ms])
    return _vfe_lockstep.BatchedVFEBound.apply(var, ls, s2, Z, key[1], X, Y)


def _laplace_key(m):
    k = m.kernel
    return ("laplace", k._kind, m._lik_kind, tuple(m.X.shape), int(k.length_scales.numel()), m.X.device)


def _laplace_groups(models):
    """[(key, indices)] of the LaplaceGP models that can share one lock-step evaluation (_laplace_lockstep.BatchedLaplaceEvidence):
    LaplaceGP's own log_likelihood over points on the GPU, grouped by (kernel kind, likelihood kind, X's shape, number of length
    scales, device) and split into chunks that fit the device's free memory; singletons stay sequential.
    key = ("laplace", kind, likelihood kind, X's shape, number of length scales, device)."""
    from . import _laplace_lockstep
    from .laplace import LaplaceGP
    groups = {}
    for i, m in enumerate(models):
        if not isinstance(m, LaplaceGP) or type(m).log_likelihood is not LaplaceGP.log_likelihood:
            continue
        if not (isinstance(m.X, torch.Tensor) and m.X.is_cuda) or not _laplace_lockstep.supported(m.X.shape[0]):
            continue
        groups.setdefault(_laplace_key(m), []).append(i)
    out = []
    for key, g in groups.items():
        out += _chunks(key, g, _capacity(_laplace_lockstep.per_model_bytes(key[3][0]), key[5], held=_held_bytes()))
    return out


def _laplace_group_inputs(ms, differentiable):
    """(X, Y, variance [B], length scales [B, nls], [m_b = mean_function(X_b)]) of one _laplace_groups / _ep_groups group: X and Y shared when
    every model holds the same tensors (restarts on one data set), else stacked"""
    m0 = ms[0]
    same_x = all(m.X.data_ptr() == m0.X.data_ptr() for m in ms)
    same_y = same_x and all(m.Y.data_ptr() == m0.Y.data_ptr() for m in ms)
    X = m0.X if same_x else torch.stack([m.X for m in ms])
    Y = m0.Y if same_y else torch.stack([m.Y for m in ms])
    var = _stacked([m.kernel.variance for m in ms], differentiable).reshape(len(ms))
    ls = _stacked([m.kernel.length_scales for m in ms], differentiable).reshape(len(ms), -1)
    if differentiable:
        means = [m.mean_function(m.X) for m in ms]
    else:
        with torch.no_grad():
            means = [m.mean_function(m.X) for m in ms]
    return X, Y, var, ls, means


def _laplace_group_evidence(ms, key, differentiable):
    """the lock-step evidences [B] of one _laplace_groups group (autograd-connected to every model's Params when differentiable)"""
    from . import _laplace_lockstep
    X, Y, var, ls, means = _laplace_group_inputs(ms, differentiable)
    return _laplace_lockstep.BatchedLaplaceEvidence.apply(X, Y, var, ls, key[1], key[2], ms, _batch_holder((key, len(ms))), *means)


def _ep_key(m):
    k = m.kernel
    link = m._lik_kind
    # (probit's moments are closed form: its models share a group whatever their likelihood's quadrature setting)
    H = 0 if link == _native.LIK_PROBIT else int(m.likelihood.num_gauss_hermite_points)
    return ("ep", k._kind, link, tuple(m.X.shape), int(k.length_scales.numel()), m.X.device, H)


def _ep_groups(models):
    """[(key, indices)] of the EPGP models that can share one lock-step evaluation (_ep_lockstep.BatchedEPEvidence): EPGP's own
    log_likelihood over points on the GPU, of a size _ep_lockstep.supported() admits, grouped and split into chunks that fit the
    device's free memory as _laplace_groups does; singletons stay sequential.
    key = ("ep", kind, likelihood kind, X's shape, number of length scales, device, H), H the number of Gauss-Hermite nodes of the
    logit link (the group's kernel stages ONE rule) and 0 for probit."""
    from . import _ep_lockstep
    from .ep import EPGP
    groups = {}
    for i, m in enumerate(models):
        if not isinstance(m, EPGP) or type(m).log_likelihood is not EPGP.log_likelihood:
            continue
        if not (isinstance(m.X, torch.Tensor) and m.X.is_cuda) or not _ep_lockstep.supported(m.X.shape[0]):
            continue
        groups.setdefault(_ep_key(m), []).append(i)
    out = []
    for key, g in groups.items():
        out += _chunks(key, g, _capacity(_ep_lockstep.per_model_bytes(key[3][0], key[4]), key[5], held=_held_bytes()))
    return out


def _ep_group_evidence(ms, key, differentiable):
    """the lock-step evidences [B] of one _ep_groups group (autograd-connected to every model's Params when differentiable)"""
    from . import _ep_lockstep
    X, Y, var, ls, means = _laplace_group_inputs(ms, differentiable)
    return _ep_lockstep.BatchedEPEvidence.apply(X, Y, var, ls, key[1], key[2], ms, _batch_holder((key, len(ms))), *means)


def _group_data(ms, differentiable=False, key=None):
    """(X, R, n_of) of a lock-step group: shared [n, d] / [n, dy] when every model holds the same tensors (restarts on one data
    set), else stacked [B, ...].  differentiable: R keeps the autograd graph of trainable mean functions.
    A ragged group (a key with sizes): X, R padded to the largest model, n_of = the sizes on the device (int32);
    otherwise n_of is None."""
    if key is not None and key.sizes is not None:
        # (data and zero-mean right-hand sides do not change between the iterations of a search: the padded stacks are kept with
        #  the group's lock-step buffers and rebuilt when a model's tensors are replaced or edited in place)
        holder = _batch_holder((key, len(ms)))
        stamp = tuple((id(m.X), m.X._version, id(m.Y), m.Y._version) for m in ms)
        cached = holder.get("ragged_data")
        if cached is not None and cached[0] == stamp:
            return cached[1], cached[2], cached[3]
        (nmax, d), B = key.shape, len(ms)
        X = torch.zeros(B, nmax, d, dtype=torch.float64, device=key.device)
        R = torch.zeros(B, nmax, key.dy, dtype=torch.float64, device=key.device)
        for b, m in enumerate(ms):
            X[b, :m.X.shape[0]] = m.X
            R[b, :m.X.shape[0]] = m.Y
        n_of = torch.tensor(key.sizes, dtype=torch.int32, device=key.device)
        holder["ragged_data"] = (stamp, X, R, n_of, [(m.X, m.Y) for m in ms])     # (holds the tensors: an id() cannot be reused)
        return X, R, n_of
    m0 = ms[0]
    same_x = all(m.X.data_ptr() == m0.X.data_ptr() for m in ms)
    zero_mean = all(type(m.mean_function) is mean_functions.Zero for m in ms)
    same_r = same_x and zero_mean and all(m.Y.data_ptr() == m0.Y.data_ptr() for m in ms)
    X = m0.X if same_x else torch.stack([m.X for m in ms])
    if same_r:
        R = m0.Y
    elif zero_mean:
        R = torch.stack([m.Y for m in ms])
    elif differentiable:
        R = torch.stack([m.Y - m.mean_function(m.X) for m in ms])
    else:
        with torch.no_grad():
            R = torch.stack([m.Y - m.mean_function(m.X) for m in ms])
    return X, R, None


def batched_log_likelihood(models, streams=None):
    """log_likelihood() of several INDEPENDENT GPR models (multi-start hyper-parameter search: one model per restart; the
    reference evaluates them one per optimiser step, gptorch/models/base.py:260-269).  No gradients (batched_loss_and_grad
    has them); returns a list of (1,) tensors, each BIT-IDENTICAL to that model's own log_likelihood().

    streams=None (default): models of one shape (kernel kind, N, D, dy) run in LOCK STEP through ONE
    gpn_lml_forward_batched call -- one assembly launch, the 128x128 leaf as a grid of B workgroups, every column pass and
    contraction as a strided-batch launch -- and the `info` words are read once at the end; a model whose factorisation
    reports info != 0 is re-evaluated through the sequential path (jitter ladder of functions.py:20-43); from
    refine_min_n() rows on every model's quadratic form is refined as log_likelihood() refines it.  Dense-K / composite
    kernels and singletons take the sequential path.

    streams = a list of HIP streams (one per model): the round-3 placement instead -- whole evaluations alternating
    over the given streams (the current stream itself gives back-to-back execution)."""
    if streams is not None:
        return _batched_on_streams(models, streams)
    _place_all(models)
    out = [None] * len(models)
    with torch.no_grad():
        pending = []
        for key, g in _lockstep_groups(models):
            ms = [models[i] for i in g]
            X, R, n_of = _group_data(ms, key=key)
            var, ls, nz = _group_hypers(ms)
            holder = _batch_holder((key, len(ms)))
            fb, terms = _ops.lml_forward_batched(key.kind, X, R, var, ls, nz, fb=holder.get("fb"),
                                                 refine=n_of is None and ms[0].X.shape[0] >= _ops.refine_min_n(), n_of=n_of)
            holder["fb"] = fb
            pending.append((g, fb, terms))
        for g, fb, terms in pending:
            info = fb.info.cpu().tolist()          # one read-back per group (synchronises the stream)
            vals = terms[:, 2:3].clone()           # ONE copy out of the shared buffers; every model gets its row of it
            for b, i in enumerate(g):
                if info[b] == 0:
                    out[i] = vals[b]
                    # (the per-model factor cache is NOT pointed at the shared buffer: the next batched call overwrites it)
        for key, g, progs in _expression_groups(models):
            ms = [models[i] for i in g]
            X, R, _ = _group_data(ms)
            nz = _stacked([m.likelihood.variance for m in ms]).reshape(len(ms))
            flat = [p for prog in progs for p in prog.params()]
            lml = _expr.BatchedExprLogLik.apply(X, R, nz, progs, _batch_holder((key, len(ms))), *flat)
            for b, i in enumerate(g):
                out[i] = lml[b:b + 1].clone()
        for key, g in _vfe_groups(models):
            elbo = _vfe_group_bound([models[i] for i in g], key, differentiable=False)
            for b, i in enumerate(g):
                out[i] = elbo[b]                                             # (VFE.log_likelihood returns a 0-dim tensor)
        for key, g in _laplace_groups(models):
            ev = _laplace_group_evidence([models[i] for i in g], key, differentiable=False)
            for b, i in enumerate(g):
                out[i] = ev[b:b + 1]                                         # (LaplaceGP.log_likelihood returns a (1,) tensor)
        for key, g in _ep_groups(models):
            ev = _ep_group_evidence([models[i] for i in g], key, differentiable=False)
            for b, i in enumerate(g):
                out[i] = ev[b:b + 1]                                         # (EPGP.log_likelihood returns a (1,) tensor)
        for i, m in enumerate(models):
            if out[i] is None:
                out[i] = m.log_likelihood()
    return out


def batched_factorise(models):
    """The factorisations the predictions of several models start from -- chol(Kyy) with L^-1 (y - m) riding along, gpr.py:104-106 --
    in LOCK STEP (cross-validation scoring: k fitted folds, each about to predict its held-out rows; the reference re-factorises
    inside every _predict call, one model at a time).  Models of one shape (kind, N, D, dy, ARD) share ONE lock-step forward into
    buffers of their own; every model's factor cache is then seeded with its slice, so its next predict_f / predict_y /
    predict_*_samples goes straight to the solve -- with the factor, and therefore the predictions, bit-identical to what the model
    would have computed alone.  A model whose factorisation needs the jitter ladder, and everything no group takes, is left to
    its own _predict.  Returns the number of models seeded."""
    _place_all(models)
    seeded = 0
    with torch.no_grad():
        for key, g in _lockstep_groups(models):
            if key.sizes is not None:                # ragged groups: a padded factor is not the layout _predict's entry points take
                continue
            ms = [models[i] for i in g]
            X, R, _ = _group_data(ms)
            fb, _terms = _ops.lml_forward_batched(key.kind, X, R, *_group_hypers(ms), fb=None)     # buffers of their own: the caches keep them
            info = fb.info.cpu()
            for b, m in enumerate(ms):
                if int(info[b]) == 0:
                    m._seed_cached_state(key.kind, m.X, fb.factor(b))
                    seeded += 1
        for key, g in _laplace_groups(models):
            # LaplaceGP folds: the mode searches in lock step into buffers of their own; every model's prediction cache gets its
            # mode, with a^ in the factor's extra row as LaplaceGP._mode_for_predict leaves it
            from . import _laplace_lockstep
            ms = [models[i] for i in g]
            X, Y, var, ls, means = _laplace_group_inputs(ms, differentiable=False)
            n = X.shape[-2]
            modes = _laplace_lockstep.find_modes(key[1], key[2], X, Y.reshape(n) if Y.dim() == 2 else Y.reshape(len(ms), n),
                                                 torch.stack([mu.reshape(n) for mu in means]), var, ls, [m._start(n) for m in ms],
                                                 [m.newton_tol for m in ms], [m.max_newton_iter for m in ms])
            for m, mode in zip(ms, modes):
                m._remember(mode)
                mode.factor.A[n, :n] = mode.a
                m._seed_cached_state(("laplace", key[1]), m.X, mode)
                seeded += 1
        for key, g in _ep_groups(models):
            # EPGP folds: the EP searches in lock step into buffers of their own; every model's prediction cache gets its sites'
            # state, with a in the factor's extra row as EPGP._mode_for_predict leaves it
            from . import _ep_lockstep
            ms = [models[i] for i in g]
            X, Y, var, ls, means = _laplace_group_inputs(ms, differentiable=False)
            n = X.shape[-2]
            sites = _ep_lockstep.find_sites_batched(key[1], key[2], X, Y.reshape(n) if Y.dim() == 2 else Y.reshape(len(ms), n),
                                                    torch.stack([mu.reshape(n) for mu in means]), var, ls, ms[0]._rule(X.device),
                                                    [m._start(n) for m in ms], [m.ep_tol for m in ms], [m.max_sweeps for m in ms],
                                                    [m.damping for m in ms])
            for m, st in zip(ms, sites):
                m._remember(st)
                st.factor.A[n, :n] = st.a
                m._seed_cached_state(("ep", key[1]), m.X, st)
                seeded += 1
    return seeded


def _has_priors(ms):
    return any(getattr(p, "prior", None) is not None for m in ms for p in m.parameters())


def _plan_groups(models):
    """the grouping of batched_loss_and_grad for a list of models: [(lock-step groups: the LML's and, with objective == "loo" in their key, the leave-one-out ones), (expression groups), (sparse groups),
    (LaplaceGP and EPGP groups: their keys begin with "laplace" / "ep")] with each group's "has priors" flag.  Shapes, kernels and priors do not change while a search runs:
    multi_start_optimize plans ONCE and hands the plan to every iteration (the grouping walks every model's parameters and, for composite kernels, rebuilds their
    expression programs: host time that a small-N iteration would spend several times over)."""
    _place_all(models)
    # leave-one-out models: groups of their own (_loo_groups), travelling in the first list with objective == "loo" in their key;
    # the other groupings do not see them (the ones no LOO group takes: their own loss(), sequentially)
    loo = [(key, g, _has_priors([models[i] for i in g])) for key, g in _loo_groups(models)]
    models = [m if getattr(m, "objective", "lml") == "lml" else None for m in models]
    return ([(key, g, _has_priors([models[i] for i in g])) for key, g in _lockstep_groups(models)] + loo,
            [(key, g, progs, _has_priors([models[i] for i in g])) for key, g, progs in _expression_groups(models)],
            [(key, g, _has_priors([models[i] for i in g])) for key, g in _vfe_groups(models)],
            [(key, g, _has_priors([models[i] for i in g])) for key, g in _laplace_groups(models) + _ep_groups(models)])


def _group_loss_and_grad(value, ms, g, priors, out, keepdim):
    """the tail of a group in batched_loss_and_grad: Model.loss (model.py:158-197) = -(value + log prior) model by model as the
    sequential code forms it, one backward for the group, every model's detached row into out ((1,) rows when keepdim: GPR;
    0-dim rows: VFE, as each class's own loss() returns them)"""
    row = (lambda t, b: t[b:b + 1]) if keepdim else (lambda t, b: t[b])
    if priors:
        # each model's own log_prior(), added to its entry of the lock-step values exactly as Model._loss adds it
        loss = (torch.cat if keepdim else torch.stack)([-(row(value, b) + m.log_prior()) for b, m in enumerate(ms)])
    else:
        loss = -(value + 0.0)                                        # model.py:_loss with an empty log prior
    if loss.requires_grad:
        loss.sum().backward()
    ld = loss.detach()
    for b, i in enumerate(g):
        out[i] = row(ld, b)


def batched_loss_and_grad(models, _plan=None):
    """`loss = m.loss(); loss.backward()` for several INDEPENDENT GPR models -- the body of the reference's optimiser step
    (gptorch/models/base.py:260-269: `closure()`), which the reference can only run one model at a time.  Gradients are
    ACCUMULATED into every trainable parameter's `.grad` exactly as backward() does; returns the list of detached (1,) loss
    tensors.

    Models of one shape (kernel kind, N, D, dy, ARD) run in LOCK STEP: one gpn_lml_forward_batched + one
    gpn_lml_backward_batched call per group (_ops.BatchedGPRLogLik), the hyper-parameters of the group stacked so that the
    transforms and their chain rule are one small launch per parameter kind.  Each model's loss AND gradients are
    BIT-IDENTICAL to its own `loss(); backward()`; a model whose factorisation fails is replayed alone through the jitter
    ladder; parameters with priors add their model's own log_prior() (model.py:158-197); sizes that refine the quadratic
    form refine it per model.  Composite / dense-K kernels and singletons take the sequential path.  Equal-shape
    GPR(objective="loo") models run in lock step too (_loo_groups, _ops.BatchedGPRLooLik: they travel in the plan's first list with
    objective == "loo" in their key), each model's loss and gradients bit-identical to its own evaluation.  Equal-shape LaplaceGP models
    run their mode searches, evidences and closed-form gradients in lock step too (_laplace_groups, models/_laplace_lockstep.py),
    each model's loss, gradients, warm-start mode and newton_stats bit-identical to its own evaluation; so do equal-shape EPGP
    models (_ep_groups, models/_ep_lockstep.py): loss, gradients, sites and ep_stats bit-identical per model."""
    plan = _plan if _plan is not None else _plan_groups(models)
    out = [None] * len(models)
    for key, g, priors in plan[0]:
        ms = [models[i] for i in g]
        X, R, n_of = _group_data(ms, differentiable=True, key=key)
        var, ls, nz = _group_hypers(ms, differentiable=True)
        holder = _batch_holder((key, len(ms)))
        if key.objective == "loo":
            # leave-one-out restarts / kernel choices of one shape: L_LOO, its closed-form gradients and -w in lock step
            _group_loss_and_grad(_ops.BatchedGPRLooLik.apply(X, R, var, ls, nz, key.kind, holder), ms, g, priors, out, True)
            continue
        if n_of is not None:
            holder["sizes"] = key.sizes
        _group_loss_and_grad(_ops.BatchedGPRLogLik.apply(X, R, var, ls, nz, key.kind, holder, n_of), ms, g, priors, out, True)
    for key, g, progs, priors in plan[1]:
        # composite kernels of one structure (the reference's example model Linear + Rbf + Constant in a multi-start search):
        # the expression's assembly and sweeps per model, everything kernel-independent once over the group
        ms = [models[i] for i in g]
        X, R, _ = _group_data(ms, differentiable=True)
        nz = _stacked([m.likelihood.variance for m in ms], differentiable=True).reshape(len(ms))
        flat = [p for prog in progs for p in prog.params()]
        lml = _expr.BatchedExprLogLik.apply(X, R, nz, progs, _batch_holder((key, len(ms))), *flat)
        _group_loss_and_grad(lml, ms, g, priors, out, True)
    for key, g, priors in plan[2]:
        # sparse models of one shape (sparse_gpr.py:108-153 in a multi-start search over inducing points / hyper-parameters)
        ms = [models[i] for i in g]
        _group_loss_and_grad(_vfe_group_bound(ms, key, differentiable=True), ms, g, priors, out, False)
    for key, g, priors in plan[3]:
        # LaplaceGP / EPGP restarts / folds of one shape: the searches, evidences and closed-form gradients in lock step
        ms = [models[i] for i in g]
        evidence = _ep_group_evidence if key[0] == "ep" else _laplace_group_evidence
        _group_loss_and_grad(evidence(ms, key, differentiable=True), ms, g, priors, out, True)
    for i, m in enumerate(models):
        if out[i] is None:
            loss = m.loss()
            if loss.requires_grad:
                loss.backward()
            out[i] = loss.detach()
    return out


_LANES = {}          # device -> two HIP streams shared by every batched call (streams= placement only)


def _batched_on_streams(models, streams):
    """whole evaluations placed on the caller's streams (see batched_log_likelihood)."""
    dev = models[0].X.device
    cur = torch.cuda.current_stream(dev)
    side = any(st is not cur for st in streams)
    if side:
        # host-side fork/join: event waits between a created stream and the legacy default stream
        # cost ~7 ms per evaluation on this runtime (tools/stream_kind_test.py waits), a host sync of an
        # idle stream costs nothing
        cur.synchronize()
    pending = []
    with torch.no_grad():
        for m, st in zip(models, streams):
            k = m._stationary()
            if k is None or m.X.shape[0] >= _ops.refine_min_n():
                # dense-K / composite kernels, and sizes at which log_likelihood() refines the quadratic form
                # (the value must not depend on which entry point computed it): sequential path
                pending.append(None)
                continue
            with torch.cuda.stream(st):
                resid = m.Y - m.mean_function(m.X)
                f = _ops.kernel_factor_async(k._kind, m.X, k.variance.transform(), k.length_scales.transform(),
                                             m.likelihood.variance.transform(), R=resid,
                                             factor=m._holder.get("factor"))
                m._holder["factor"] = f
                pending.append((f, f.lml_terms(), st))
        out = []
        for m, p in zip(models, pending):
            ok = False
            if p is not None:
                with torch.cuda.stream(p[2]):
                    ok = int(p[0].info.item()) == 0        # synchronises that model's stream
            out.append(p[1][2:3] if ok else m.log_likelihood())
    return out


def two_lane_streams(models):
    """the round-3 default placement of batched_log_likelihood(streams=...): the models alternate between two internal streams."""
    dev = models[0].X.device
    if dev not in _LANES:
        _LANES[dev] = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    return [_LANES[dev][i % 2] for i in range(len(models))]
