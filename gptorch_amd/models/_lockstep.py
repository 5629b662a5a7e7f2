"""
Several INDEPENDENT models evaluated in lock step: which models can share a call (the group keys and their memory-capacity
rule), the buffers a group keeps between calls, and the public batched entry points batched_log_likelihood,
batched_loss_and_grad and batched_factorise, which are loops over FAMILIES: one entry per kind of group.
(GPR and VFE are imported where they are needed: models/gpr.py imports this module.)
"""
import collections
from typing import Any, Callable, NamedTuple, Optional

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


# The other families' keys.  Each begins with its family's name: named tuples of different classes compare as plain tuples, and
# the key names the group's cached buffers.
class ExprKey(NamedTuple):
    tag: str
    signature: tuple                  # _expr.Program.signature(): the composite kernel's structure
    shape: tuple
    dy: int
    device: torch.device


class VFEKey(NamedTuple):
    tag: str
    kind: str
    shape: tuple
    dy: int
    nls: int
    z_shape: tuple                    # Z's (number of inducing points, d)
    device: torch.device


class SiteKey(NamedTuple):
    """LaplaceGP and EPGP groups"""
    tag: str
    kind: str
    lik_kind: int
    shape: tuple
    nls: int
    device: torch.device
    H: Optional[int] = None           # EPGP: Gauss-Hermite nodes of the logit link (a group's kernel stages ONE rule), 0 for probit


class Group(NamedTuple):
    """the models of one list that share a lock-step call"""
    family: "Family"
    key: tuple                        # (key, number of models) names the group's cached buffers
    indices: list
    payload: Any = None               # the expression family's programs, one per model
    priors: Optional[bool] = None     # in a plan: whether any parameter of the group's models has a prior


class Family(NamedTuple):
    """one kind of lock-step group (FAMILIES)"""
    name: str
    find: Callable                    # the grouping function: models -> [(key, indices[, payload])]
    value: Callable                   # (ms, group, differentiable) -> the [B] lock-step values (see batched_log_likelihood)
    keepdim: bool                     # rows as the class's own loss() returns them: (1,), else 0-dim
    seed: Optional[Callable] = None   # (ms, group) -> number of models whose prediction caches it seeded
    objective: str = "lml"            # the GPR.objective its groups evaluate ("lml": the value is log_likelihood())
    held: tuple = ()                  # the tensors a group's holder keeps beside its FactorBatch "fb"
    stacked: bool = False             # find takes for_grad=True: groups for multi_start_optimize's stacked-parameter loop
    captured: bool = True             # under multi_start_optimize(capture=True) its models may share an evaluation

    def groups(self, models, for_grad=False):
        if for_grad:
            return [Group(self, *found) for found in self.find(models, for_grad=True)] if self.stacked else []
        return [Group(self, *found) for found in self.find(models)]


# Lock-step buffers reused between calls (a search calls batched_log_likelihood / batched_loss_and_grad once per optimiser
# step): keyed by the FULL group key + batch size -- two groups of one call can never share an entry (round-4 advice: keyed
# by (device, batch, n, dy) only, two groups of equal count / N / dy but different kernel kind or ARD shared one buffer and
# the first group read the second group's results) -- least recently used first out, bounded in entries and bytes;
# release_batch_buffers() drops them all.
_BATCH_BUFFERS = collections.OrderedDict()    # (group key, batch) -> holder dict {"fb": _ops.FactorBatch}
BATCH_BUFFER_MAX_ENTRIES = 4
BATCH_BUFFER_MAX_BYTES = 48 << 30


def _held_bytes():
    # (every holder's FactorBatch -- the inversion's workspace is its _backward_work -- and what the families say their holders
    #  keep beside it: _HELD_BESIDE_FB, from FAMILIES)
    return sum(v["fb"].nbytes() for v in _BATCH_BUFFERS.values() if "fb" in v) + \
        sum(8 * v[name].numel() for v in _BATCH_BUFFERS.values() for name in _HELD_BESIDE_FB if v.get(name) is not None)


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


def three_padded_matrices_bytes(n):
    """3 padded N x N matrices: what a GPR or LaplaceGP model of n rows holds in a lock-step call (factor + the backward's two)"""
    ld = -(-int(n) // 128) * 128 + 128
    return 3 * 8 * (ld + 16) * ld


def _chunked(groups, per_model, held=True):
    """{key: indices} as [(key, indices)] chunks that fit the device's free memory at per_model(key) bytes a model (held: the cache's
    buffers count as free); singletons fall to the sequential path"""
    out = []
    for key, g in groups.items():
        cap = _capacity(per_model(key), key.device, held=_held_bytes() if held else 0)
        out += [(key, g[at:at + cap]) for at in range(0, len(g), cap) if len(g[at:at + cap]) >= 2]
    return out


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
        out += _chunked({key: g}, lambda key: three_padded_matrices_bytes(key.shape[0]))
    for (common, _regime), g in pool.items():
        g = sorted(g, key=lambda i: (-models[i].X.shape[0], i))
        at = 0
        while at < len(g):
            nmax = models[g[at]].X.shape[0]
            end = at + 1
            cap = _capacity(three_padded_matrices_bytes(nmax), common.device, held=_held_bytes())
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
    return _chunked(groups, lambda key: _loo_lockstep.per_model_bytes(key.shape[0], key.dy, key.nls))


def _expression_groups(models):
    """[(ExprKey, indices, programs)] of the GPR models over COMPOSITE kernels of one structure (equal _expr.Program.signature(),
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
        key = ExprKey("expr", prog.signature(), tuple(m.X.shape), m.Y.shape[1], m.X.device)
        groups.setdefault(key, ([], []))
        groups[key][0].append(i)
        groups[key][1].append(prog)
    return [(key, g, progs) for key, (g, progs) in groups.items() if len(g) >= 2]


def _vfe_groups(models):
    """[(VFEKey, indices)] of the VFE models (sparse_gpr.py:108-153) that can share one lock-step evaluation
    (_vfe_lockstep.BatchedVFEBound): one native stationary kind, equal (N, D, dy, M, ARD), on one device, in the single-chunk regime
    (_vfe_lockstep.supported); split into chunks that fit the device's free memory (the cache's buffers do not count as free)."""
    from . import _vfe_lockstep
    from .sparse_gpr import VFE
    groups = {}
    for i, m in enumerate(models):
        if not isinstance(m, VFE) or type(m).log_likelihood is not VFE.log_likelihood or type(m)._bound is not VFE._bound:
            continue
        k = m._native_kernel()
        if k is None or not m.X.is_cuda or not _vfe_lockstep.supported(m.X.shape[0], m.Z.shape[0]):
            continue
        key = VFEKey("vfe", k._kind, tuple(m.X.shape), m.Y.shape[1], int(k.length_scales.numel()), tuple(m.Z.shape), m.X.device)
        groups.setdefault(key, []).append(i)
    return _chunked(groups, lambda key: _vfe_lockstep.per_model_bytes(key.shape[0], key.z_shape[0], key.dy), held=False)


def _shared_or_stacked(ms, with_y=True):
    """(X, Y) of a group: the models' own [n, d] / [n, dy] when every model holds the same tensors (restarts on one data set; Y
    only where X is shared too), else stacked [B, ...]"""
    m0 = ms[0]
    same_x = all(m.X.data_ptr() == m0.X.data_ptr() for m in ms)
    X = m0.X if same_x else torch.stack([m.X for m in ms])
    if not with_y:
        return X, None
    return X, m0.Y if same_x and all(m.Y.data_ptr() == m0.Y.data_ptr() for m in ms) else torch.stack([m.Y for m in ms])


def _vfe_group_bound(ms, group, differentiable):
    """the lock-step bounds [B] of one _vfe_groups group (autograd-connected to every model's Params when differentiable): sparse
    models of one shape (sparse_gpr.py:108-153 in a multi-start search over inducing points / hyper-parameters)"""
    from . import _vfe_lockstep
    X, Y = _shared_or_stacked(ms)                                        # sparse_gpr.py:125 quirk: err = Y (Zero mean only)
    var, ls, s2 = _group_hypers(ms, differentiable)
    Z = torch.stack([m.Z for m in ms]) if differentiable else torch.stack([m.Z.data for m in ms])
    return _vfe_lockstep.BatchedVFEBound.apply(var, ls, s2, Z, group.key.kind, X, Y)


def _laplace_key(m):
    k = m.kernel
    return SiteKey("laplace", k._kind, m._lik_kind, tuple(m.X.shape), int(k.length_scales.numel()), m.X.device)


def _ep_key(m):
    k = m.kernel
    link = m._lik_kind
    # (probit's moments are closed form: its models share a group whatever their likelihood's quadrature setting)
    H = 0 if link == _native.LIK_PROBIT else int(m.likelihood.num_gauss_hermite_points)
    return SiteKey("ep", k._kind, link, tuple(m.X.shape), int(k.length_scales.numel()), m.X.device, H)


def _family_module(tag):
    """the lock-step module of a SiteKey's family; each gives MODEL, supported, per_model_bytes, search and its node"""
    from . import _ep_lockstep, _laplace_lockstep
    return {"laplace": _laplace_lockstep, "ep": _ep_lockstep}[tag]


def _site_groups(models, tag, key_of):
    """[(SiteKey, indices)] of the family's (LaplaceGP / EPGP) models that can share one lock-step evaluation: the class's own
    log_likelihood over points on the GPU, of a size the family's supported() admits, by key_of, in chunks that fit the device's free
    memory"""
    lockstep = _family_module(tag)
    cls = lockstep.MODEL
    groups = {}
    for i, m in enumerate(models):
        if not isinstance(m, cls) or type(m).log_likelihood is not cls.log_likelihood:
            continue
        if not (isinstance(m.X, torch.Tensor) and m.X.is_cuda) or not lockstep.supported(m.X.shape[0]):
            continue
        groups.setdefault(key_of(m), []).append(i)
    return _chunked(groups, lambda key: lockstep.per_model_bytes(key.shape[0], key.nls))


def _laplace_groups(models):
    """[(SiteKey, indices)]: _site_groups of the LaplaceGP models (_laplace_lockstep.BatchedLaplaceEvidence)"""
    return _site_groups(models, "laplace", _laplace_key)


def _ep_groups(models):
    """[(SiteKey, indices)]: _site_groups of the EPGP models (_ep_lockstep.BatchedEPEvidence)"""
    return _site_groups(models, "ep", _ep_key)


def _site_group_inputs(ms, differentiable):
    """(X, Y, variance [B], length scales [B, nls], [m_b = mean_function(X_b)]) of one _laplace_groups / _ep_groups group"""
    X, Y = _shared_or_stacked(ms)
    var = _stacked([m.kernel.variance for m in ms], differentiable).reshape(len(ms))
    ls = _stacked([m.kernel.length_scales for m in ms], differentiable).reshape(len(ms), -1)
    with torch.set_grad_enabled(differentiable and torch.is_grad_enabled()):
        means = [m.mean_function(m.X) for m in ms]
    return X, Y, var, ls, means


def _site_group_evidence(ms, group, differentiable):
    """the lock-step evidences [B] of one LaplaceGP / EPGP group by its family's node (autograd-connected when differentiable)"""
    key = group.key
    X, Y, var, ls, means = _site_group_inputs(ms, differentiable)
    return _family_module(key.tag).NODE.apply(X, Y, var, ls, key.kind, key.lik_kind, ms, _batch_holder((key, len(ms))), *means)


_laplace_group_evidence = _ep_group_evidence = _site_group_evidence       # (the names each family's tests and tools call it by)


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
    zero_mean = all(type(m.mean_function) is mean_functions.Zero for m in ms)
    X, R = _shared_or_stacked(ms, with_y=zero_mean)                      # (zero means: the residuals are Y itself)
    if not zero_mean:
        with torch.set_grad_enabled(differentiable and torch.is_grad_enabled()):
            R = torch.stack([m.Y - m.mean_function(m.X) for m in ms])
    return X, R, None


def _lml_value(ms, group, differentiable):
    key = group.key
    X, R, n_of = _group_data(ms, differentiable, key=key)
    var, ls, nz = _group_hypers(ms, differentiable)
    holder = _batch_holder((key, len(ms)))
    if differentiable:
        if n_of is not None:
            holder["sizes"] = key.sizes
        return _ops.BatchedGPRLogLik.apply(X, R, var, ls, nz, key.kind, holder, n_of)
    fb, terms = _ops.lml_forward_batched(key.kind, X, R, var, ls, nz, fb=holder.get("fb"),
                                         refine=n_of is None and ms[0].X.shape[0] >= _ops.refine_min_n(), n_of=n_of)
    holder["fb"] = fb

    def finish():
        """-> every model's (1,) row; None where the factorisation reported info != 0 (the sequential path's jitter ladder)"""
        info = fb.info.cpu().tolist()          # one read-back per group (synchronises the stream)
        vals = terms[:, 2:3].clone()           # ONE copy out of the shared buffers; every model gets its row of it
        # (the per-model factor cache is NOT pointed at the shared buffer: the next batched call overwrites it)
        return [vals[b] if info[b] == 0 else None for b in range(len(ms))]
    return finish


def _lml_seed(ms, group):
    key = group.key
    if key.sizes is not None:                  # ragged groups: a padded factor is not the layout _predict's entry points take
        return 0
    X, R, _ = _group_data(ms)
    fb, _terms = _ops.lml_forward_batched(key.kind, X, R, *_group_hypers(ms), fb=None)     # buffers of their own: the caches keep them
    info = fb.info.cpu()
    ok = [b for b in range(len(ms)) if int(info[b]) == 0]
    for b in ok:
        ms[b]._seed_cached_state(key.kind, ms[b].X, fb.factor(b))
    return len(ok)


def _loo_value(ms, group, differentiable):
    """leave-one-out restarts / kernel choices of one shape: L_LOO, its closed-form gradients and -w in lock step"""
    key = group.key
    X, R, _ = _group_data(ms, differentiable, key=key)
    var, ls, nz = _group_hypers(ms, differentiable)
    return _ops.BatchedGPRLooLik.apply(X, R, var, ls, nz, key.kind, _batch_holder((key, len(ms))))


def _expr_value(ms, group, differentiable):
    """composite kernels of one structure (the reference's example model Linear + Rbf + Constant in a multi-start search): the
    expression's assembly and sweeps per model, everything kernel-independent once over the group"""
    X, R, _ = _group_data(ms, differentiable)
    nz = _stacked([m.likelihood.variance for m in ms], differentiable).reshape(len(ms))
    flat = [p for prog in group.payload for p in prog.params()]
    lml = _expr.BatchedExprLogLik.apply(X, R, nz, group.payload, _batch_holder((group.key, len(ms))), *flat)
    return lml if differentiable else [lml[b:b + 1].clone() for b in range(len(ms))]       # (rows: every model its own copy)


def _site_seed(ms, group):
    """LaplaceGP / EPGP folds: the searches (mode / sites) in lock step into buffers of their own; every model's prediction cache
    gets its state, with a in the factor's extra row as the class's _mode_for_predict leaves it"""
    key = group.key
    X, Y, var, ls, means = _site_group_inputs(ms, differentiable=False)
    n = X.shape[-2]
    stack = _family_module(key.tag).search(ms, key.kind, key.lik_kind, X, Y.reshape(n) if Y.dim() == 2 else Y.reshape(len(ms), n),
                                           torch.stack([mu.reshape(n) for mu in means]), var, ls, [m._start(n) for m in ms])
    for m, state in zip(ms, stack.states):
        m._remember(state)
        state.factor.A[n, :n] = state.a
        m._seed_cached_state((key.tag, key.kind), m.X, state)
    return len(ms)


# Every kind of lock-step group, in the order in which the entry points evaluate them (it fixes the LRU order of _BATCH_BUFFERS
# and the order of gradient accumulation for models that share Param objects).  A new family is one more entry.
FAMILIES = (
    Family("lml", _lockstep_groups, _lml_value, True, seed=_lml_seed, stacked=True),
    # (held: the right-hand sides of w, Q and the sweep's partials)
    Family("loo", _loo_groups, _loo_value, True, objective="loo", held=("loo_rhs", "loo_q", "loo_sweep")),
    Family("expr", _expression_groups, _expr_value, True),
    Family("vfe", _vfe_groups, _vfe_group_bound, False),
    # (capture=True: LaplaceGP and EPGP models keep their own optimize())
    Family("laplace", _laplace_groups, _site_group_evidence, True, seed=_site_seed, captured=False),
    Family("ep", _ep_groups, _site_group_evidence, True, seed=_site_seed, captured=False),
)
_HELD_BESIDE_FB = tuple(name for family in FAMILIES for name in family.held)


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
        for family in FAMILIES:
            if family.objective != "lml":          # (log_likelihood() is the LML whatever a model fits)
                continue
            # Without gradients a value is the [B] tensor, the models' rows already cut, or a finisher that returns the rows (None:
            # left to the model's own log_likelihood() below): EVERY group of the family is launched before the first finisher runs
            launched = [(group, family.value([models[i] for i in group.indices], group, False)) for group in family.groups(models)]
            for group, value in launched:
                rows = value() if callable(value) else value
                for b, i in enumerate(group.indices):
                    out[i] = rows[b] if isinstance(rows, list) else _row(rows, b, family.keepdim)
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
        for family in FAMILIES:
            if family.seed is not None:
                for group in family.groups(models):
                    seeded += family.seed([models[i] for i in group.indices], group)
    return seeded


def _has_priors(ms):
    return any(getattr(p, "prior", None) is not None for m in ms for p in m.parameters())


def _plan_groups(models):
    """the grouping of batched_loss_and_grad for a list of models: one flat [Group] in the order of FAMILIES, each group with its
    "has priors" flag; a family sees the models whose objective it evaluates (a model without one: "lml").  Shapes, kernels and
    priors do not change while a search runs: multi_start_optimize plans ONCE and hands the plan to every iteration (the grouping
    walks every model's parameters and rebuilds expression programs: host time a small-N iteration would spend several times over)."""
    _place_all(models)
    plan = []
    objectives = [getattr(m, "objective", "lml") for m in models]          # (once: a miss on a model without the attribute is slow)
    for family in FAMILIES:
        own = [m if objective == family.objective else None for m, objective in zip(models, objectives)]
        plan += [group._replace(priors=_has_priors([models[i] for i in group.indices])) for group in family.groups(own)]
    return plan


def _row(t, b, keepdim):
    return t[b:b + 1] if keepdim else t[b]


def _group_loss_and_grad(value, ms, g, priors, out, keepdim):
    """the tail of a group in batched_loss_and_grad: Model.loss (model.py:158-197) = -(value + log prior) model by model as the
    sequential code forms it, one backward for the group, every model's detached row into out ((1,) rows when keepdim: GPR;
    0-dim rows: VFE, as each class's own loss() returns them)"""
    if priors:
        # each model's own log_prior(), added to its entry of the lock-step values exactly as Model._loss adds it
        loss = (torch.cat if keepdim else torch.stack)([-(_row(value, b, keepdim) + m.log_prior()) for b, m in enumerate(ms)])
    else:
        loss = -(value + 0.0)                                        # model.py:_loss with an empty log prior
    if loss.requires_grad:
        loss.sum().backward()
    ld = loss.detach()
    for b, i in enumerate(g):
        out[i] = _row(ld, b, keepdim)


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
    GPR(objective="loo") models run in lock step too (_loo_groups, _ops.BatchedGPRLooLik: the plan's "loo" groups), each model's
    loss and gradients bit-identical to its own evaluation.  Equal-shape LaplaceGP models
    run their mode searches, evidences and closed-form gradients in lock step too (_laplace_groups, models/_laplace_lockstep.py),
    each model's loss, gradients, warm-start mode and newton_stats bit-identical to its own evaluation; so do equal-shape EPGP
    models (_ep_groups, models/_ep_lockstep.py): loss, gradients, sites and ep_stats bit-identical per model."""
    plan = _plan if _plan is not None else _plan_groups(models)
    out = [None] * len(models)
    for group in plan:
        ms = [models[i] for i in group.indices]
        _group_loss_and_grad(group.family.value(ms, group, True), ms, group.indices, group.priors, out, group.family.keepdim)
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
