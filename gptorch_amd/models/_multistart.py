"""
Several INDEPENDENT restarts optimised at once (multi_start_optimize): torch optimisers over stacked parameters or one optimiser
per model with a shared lock-step evaluation (models/_lockstep.py), scipy methods with every restart's `minimize` in its own
host thread and one batched evaluation per round.
"""
import torch

from .. import _ops
from ._lockstep import (FAMILIES, _group_data, _group_param_lists, _lockstep_groups, _place_all, _plan_groups, _shared_transform,
                        batched_loss_and_grad, release_batch_buffers)
from .base import _SCIPY_METHODS, _TORCH_DEFAULT_LR


# scipy methods whose `minimize` holds a module-wide lock while it runs (one restart at a time whatever we do)
_SCIPY_SERIAL_METHODS = ("COBYLA",)
_MULTI_START_STALL_S = 2.0       # a round of the scipy multi-start stops waiting for silent restarts after this long
_MULTI_START_JOIN_S = 10.0


class _MultiStartAborted(RuntimeError):
    """raised inside a restart's objective when the multi-start search it belongs to has ended (interrupt, error)."""


def _multi_start_scipy(models, method, max_iter, verbose):
    """scipy.optimize.minimize for every model AT ONCE (base.py:298-320; what examples/regression_1d.py:53 and the
    reference's notebooks run is L-BFGS-B): each restart's `minimize` runs in its own host thread and only ever waits -- its
    `fun(x)` posts the parameter vector it wants evaluated and sleeps; the calling thread collects one request per
    still-running restart, evaluates ALL of them in one batched_loss_and_grad call (lock-step groups + sequential rest),
    and hands every restart its (loss, gradient).  Line searches make the restarts ask for different numbers of
    evaluations, and restarts finish at different iterations: a round simply covers whoever is still running.  Each
    restart sees exactly the values Model._loss_and_grad (model.py:123-133) would have given it -- bit for bit -- so its
    iterates, its result and its printed losses are those of its own optimize(); only the order in which the restarts'
    "loss: ..." lines interleave differs.  -> list of scipy OptimizeResult."""
    import threading
    import numpy as np
    from scipy.optimize import minimize
    B = len(models)
    if method in _SCIPY_SERIAL_METHODS:
        # scipy runs these under a module-wide lock (COBYLA: scipy.optimize._cobyla_py._module_lock): a second restart's
        # `minimize` cannot even start while the first one sits in its objective, so the restarts cannot post requests together.
        # One after the other through each model's own optimize() -- what the reference does (base.py:298-320).
        return [m.optimize(method=method, max_iter=max_iter, verbose=verbose) for m in models]
    cond = threading.Condition()
    pending, answers = {}, {}
    done = [False] * B
    results = [None] * B
    state = {"abort": None}
    x0 = [m._get_param_array() for m in models]

    def make_fun(i):
        def fun(x):
            with cond:
                if state["abort"] is not None:
                    raise _MultiStartAborted(state["abort"])
                pending[i] = np.array(x, dtype=np.float64, copy=True)
                cond.notify_all()
                while i not in answers and state["abort"] is None:
                    cond.wait()
                if i not in answers:
                    pending.pop(i, None)
                    raise _MultiStartAborted(state["abort"])
                ans = answers.pop(i)
            if isinstance(ans, BaseException):
                raise ans
            return ans
        return fun

    def worker(i):
        try:
            results[i] = minimize(fun=make_fun(i), x0=x0[i], method=method, jac=True, tol=None, callback=None,
                                  options=dict(disp=verbose, maxiter=max_iter))
        except BaseException as exc:             # delivered to the caller after every restart has finished
            results[i] = exc
        finally:
            with cond:
                done[i] = True
                cond.notify_all()

    threads = [threading.Thread(target=worker, args=(i,), daemon=True) for i in range(B)]
    for t in threads:
        t.start()
    try:
        while True:
            with cond:
                stalled = False
                while True:
                    active = [i for i in range(B) if not done[i]]
                    if not active or all(i in pending for i in active):
                        break
                    # a restart that neither finishes nor posts (a method that serialises inside scipy, a callback that blocks):
                    # after the stall time-out the round covers whoever HAS posted -- never a dead wait
                    if not cond.wait(timeout=_MULTI_START_STALL_S) and pending:
                        stalled = True
                        break
                if not active:
                    break
                batch = {i: pending.pop(i) for i in (active if not stalled else sorted(pending))}
            idx = sorted(batch)
            out = {}
            try:
                # Model._loss_and_grad (model.py:123-133) for all requests of the round at once.  The requested vectors travel to
                # the device as ONE copy and every parameter becomes a slice of it (model.py:66-76 makes one tensor per parameter:
                # 3 small copies per model and round); the gradients come back as ONE copy.
                dev = models[idx[0]].X.device
                flat = torch.as_tensor(np.concatenate([batch[i] for i in idx]), dtype=torch.float64).to(dev)
                at = 0
                for i in idx:
                    for p in models[i].parameters():
                        if p.requires_grad:
                            nxt = at + p.numel()
                            p.data = flat[at:nxt].reshape(p.shape)
                            at = nxt
                        p.grad = None                    # (a fresh gradient: what zeroing + accumulating gives)
                losses = batched_loss_and_grad([models[i] for i in idx])
                trainable = [[p for p in models[i].parameters() if p.requires_grad] for i in idx]
                allg = torch.cat([p.grad.reshape(-1) for ps in trainable for p in ps] + [l.reshape(-1) for l in losses]).cpu().numpy()
                lvals = allg[len(allg) - len(idx):]
                at = 0
                staged = {}
                for k, i in enumerate(idx):
                    cnt = sum(p.numel() for p in trainable[k])
                    staged[i] = (float(lvals[k]), np.array(allg[at:at + cnt]))
                    at += cnt
                for i in idx:                            # (nothing is printed before the whole round has its values)
                    value, grad = staged[i]
                    print("loss: %s" % value)
                    finite = np.isfinite(grad)
                    if np.all(finite):
                        out[i] = (value, grad.astype(np.float64))
                    else:
                        print("Warning: inf or nan in gradient: replacing with zeros")
                        out[i] = (value, np.where(finite, grad, 0.0).astype(np.float64))
            except Exception:
                # one request of the round failed (e.g. the jitter ladder ran out for one model): evaluate them one by one so
                # that only the restart it belongs to sees the exception.  (KeyboardInterrupt / SystemExit are not caught here:
                # they end the whole search through the `finally` below.)
                out = {}
                for i in idx:
                    try:
                        out[i] = models[i]._loss_and_grad(batch[i])
                    except Exception as exc:
                        out[i] = exc
            with cond:
                answers.update(out)
                cond.notify_all()
    except BaseException as exc:
        with cond:
            state["abort"] = exc
        raise
    finally:
        # whatever ended the collecting loop, no worker stays behind waiting for an answer: every pending and every future
        # request of a restart that is still running is answered with _MultiStartAborted, its `minimize` unwinds, its thread ends
        with cond:
            if state["abort"] is None and not all(done):
                state["abort"] = RuntimeError("multi-start search ended early")
            cond.notify_all()
        for t in threads:
            t.join(timeout=_MULTI_START_JOIN_S)
    for r in results:
        if isinstance(r, BaseException):
            raise r
    return results


STACKED_MAX_N = 2048      # multi_start_optimize(stacked=None): stacked parameter tensors below this many rows, one optimiser per model from it on


def multi_start_optimize(models, method="Adam", max_iter=2000, verbose=False, learning_rate=None, stacked=None, capture=False):
    """GPModel.optimize (gptorch/models/base.py:111-296) for several INDEPENDENT restarts at once: every iteration is ONE
    lock-step loss + backward over each group of equally shaped models (see batched_loss_and_grad) and ONE optimiser step
    on the group's STACKED raw parameters -- the torch optimisers the reference offers are elementwise (all but LBFGS), so
    every restart follows the trajectory its own `optimize()` would.  Given equal parameters the losses and gradients are
    bit-identical to the sequential ones; the optimiser step itself is PyTorch's multi-tensor kernel, which rounds
    `p + value * (a / b)` with or without a fused multiply-add depending on a tensor's size and alignment (measured: 1 ulp
    on a parameter after 2 Adam steps for [4, 1] against [1]), so trajectories agree to ~1e-12 relative, not bit for bit.
    stacked=False: no stacked parameter tensors at all -- every model keeps its own optimiser and only the evaluation is shared:
    trajectories BIT-IDENTICAL to each model's own optimize(), at one optimiser step per model and iteration of host work
    (C1 x 64: 6 ms per iteration instead of 1; immaterial from N = 2048 on).
    stacked=None (the default): the bitwise mode wherever it is free -- groups of models with at least STACKED_MAX_N (2048) rows
    keep one optimiser per model, smaller ones are stacked.
    capture=True: the stacked groups' iteration -- transforms, lock-step evaluation, closed-form backward, the optimiser's
    `capturable` step, the loss row -- is captured into ONE hipGraph after three eager steps and replayed (GPModel.optimize(
    capture=True) for B restarts at once: base.py:260-269 without a host round trip per iteration); `info != 0` is OR-ed into a
    device flag read every 25 replays, and a chunk that saw one is rolled back and repeated eagerly through the jitter ladder.
    Trajectories agree with the uncaptured stacked loop to rounding (the optimiser's bias corrections are formed on the device).
    Returns (losses [len(models), max_iter] numpy, seconds).  The models' Params hold the final values afterwards.

    Stacked groups: as batched_loss_and_grad's stationary groups, and additionally every model of the group trains the same
    subset of (variance, length_scales, noise) with a shared transform, no priors and no trainable mean function.  Everything
    else that batched_loss_and_grad can still evaluate together (composite kernels of one structure, models with priors or
    trainable means) keeps ONE OPTIMISER PER MODEL and shares only the evaluation: those trajectories are bit-identical to
    each model's own optimize().  method="LBFGS" (a closure-driven line search per model) and models nothing can be shared
    with are optimised one after the other by their own optimize().

    scipy methods ("L-BFGS-B", "CG", "BFGS" ...: base.py:203-215, 298-320): every restart's scipy.optimize.minimize runs at
    once and each round of function evaluations is ONE batched_loss_and_grad call (_multi_start_scipy); returns
    (list of scipy results, seconds) -- each bit-identical to the model's own optimize(method=...)."""
    import time
    import numpy as np
    _place_all(models)
    if method in _SCIPY_METHODS:
        print("Scipy.optimize.minimize...")
        tic = time.time()
        try:
            return _multi_start_scipy(models, method, max_iter, verbose), time.time() - tic
        finally:
            release_batch_buffers()
    if learning_rate is None and method in _TORCH_DEFAULT_LR:
        learning_rate = _TORCH_DEFAULT_LR[method]
    losses = np.zeros((len(models), max_iter))
    done = [False] * len(models)
    tic = time.time()
    groups = _lockstep_groups(models, for_grad=True) if (stacked is not False and method in _TORCH_DEFAULT_LR and method != "LBFGS") else []
    if stacked is None:
        groups = [(key, g) for key, g in groups if key.shape[0] < STACKED_MAX_N]
    for key, g in groups:
        ms = [models[i] for i in g]
        B = len(ms)
        plists = _group_param_lists(ms)
        transforms = [_shared_transform(pl) for pl in plists]
        flags = [{bool(p.requires_grad) for p in pl} for pl in plists]
        mean_trainable = any(p.requires_grad for m in ms for p in m.mean_function.parameters())
        if any(t is None for t in transforms) or any(len(f) != 1 for f in flags) or mean_trainable:
            continue
        X, R, _ = _group_data(ms)
        raws = [torch.nn.Parameter(torch.stack([p.data for p in pl]), requires_grad=f.pop()) for pl, f in zip(plists, flags)]
        trainable = [r for r in raws if r.requires_grad]
        if not trainable:
            continue                     # nothing to optimise in lock step: each model's own optimize() reports as the reference does
        holder = {}
        dev_losses = torch.empty(max_iter, B, dtype=torch.float64, device=X.device)
        print("multi_start_optimize: %d x %s in lock step via %s" % (B, ms[0].__class__.__name__, method))

        def step(optimizer, idx, set_to_none=False):
            optimizer.zero_grad(set_to_none=set_to_none)
            var, ls, nz = (t(r) for t, r in zip(transforms, raws))
            lml = _ops.BatchedGPRLogLik.apply(X, R, var.reshape(B), ls.reshape(B, -1), nz.reshape(B), key.kind, holder)
            loss = -(lml + 0.0)
            loss.sum().backward()
            optimizer.step()
            if idx is not None:
                dev_losses[idx] = loss.detach()
            return loss
        if capture:
            # the iteration as ONE hipGraph after GPModel.CAPTURE_WARMUP eager steps (the single-model form: GPModel._optimize_captured)
            optimizer = ms[0]._captured_loop(trainable, lambda: ms[0]._make_optimizer(method, trainable, learning_rate),
                                             lambda optimizer, idx: step(optimizer, idx, set_to_none=True), dev_losses, max_iter)
            if verbose:                                # (the replays print nothing: the lines of the ordinary loop, afterwards)
                for idx, row in enumerate(dev_losses.tolist()):
                    print("Iter: %d\tLoss: %s" % (idx, row))
        else:
            optimizer = ms[0]._make_optimizer(method, trainable, learning_rate)
            for idx in range(max_iter):
                step(optimizer, idx)
                if verbose:
                    print("Iter: %d\tLoss: %s" % (idx, dev_losses[idx].tolist()))
        losses[g, :] = dev_losses.t().cpu().numpy()
        with torch.no_grad():
            for pl, r in zip(plists, raws):
                for b, p in enumerate(pl):
                    p.data = r.data[b].clone()
        for i in g:
            done[i] = True
    rest = [i for i in range(len(models)) if not done[i]]
    rest_models = [models[i] for i in rest]
    # (any family that evaluates log_likelihood() taking a group of the list AS IT IS -- not of the plan's view, in which a
    #  leave-one-out model enters LOO groups only; capture=True: LaplaceGP and EPGP models keep their own optimize())
    sharing = [f for f in FAMILIES if f.objective == "lml" and (f.captured or not capture)]
    if method in _TORCH_DEFAULT_LR and method != "LBFGS" and len(rest) >= 2 and any(f.groups(rest_models) for f in sharing):
        # What cannot share a stacked parameter tensor (composite kernels, priors, trainable mean functions, mixed frozen
        # parameters) still shares the EVALUATION: every model keeps its own optimiser over its own parameters -- exactly the
        # objects and tensor layouts of its own optimize(), so its trajectory is bit-identical -- and each iteration is one
        # batched_loss_and_grad over all of them (base.py:260-269: zero_grad, loss, backward, step).
        opts = []
        for m in rest_models:
            m._auto_place()
        plist = [p for m in rest_models for p in m.parameters() if p.requires_grad]
        if len({id(p) for p in plist}) == len(plist):
            # ONE optimiser object over every model's own parameter tensors: the torch optimisers are elementwise per tensor and
            # their multi-tensor kernels treat every tensor of the list by itself, so each model's update is what its own
            # optimiser would do -- bit for bit -- at one step() call per iteration instead of one per model
            shared = rest_models[0]._make_optimizer(method, plist, learning_rate)
            for m in rest_models:
                m.optimizer = shared
            opts.append(shared)
        else:                                   # models that share Param objects: every model's own optimiser, as optimize() would
            for m in rest_models:
                m.optimizer = m._make_optimizer(method, [p for p in m.parameters() if p.requires_grad], learning_rate)
                opts.append(m.optimizer)
        print("multi_start_optimize: %d models, one lock-step evaluation per iteration, via %s" % (len(rest), method))
        plan = _plan_groups(rest_models)              # (shapes, kernels and priors are fixed while the search runs)
        for idx in range(max_iter):
            for o in opts:
                o.zero_grad()
            out = batched_loss_and_grad(rest_models, _plan=plan)
            for o in opts:
                o.step()
            vals = torch.cat([l.reshape(-1) for l in out]).cpu().numpy()
            losses[rest, idx] = vals
            if verbose:
                print("Iter: %d\tLoss: %s" % (idx, vals.tolist()))
        for i in rest:
            done[i] = True
    for i, m in enumerate(models):
        if not done[i]:
            res = m.optimize(method=method, max_iter=max_iter, verbose=verbose, learning_rate=learning_rate)
            if isinstance(res, tuple):
                losses[i, :len(res[0])] = res[0]
    release_batch_buffers()          # the search is over: its lock-step buffers (B factors + backward workspaces) go back to the allocator
    return losses, time.time() - tic
