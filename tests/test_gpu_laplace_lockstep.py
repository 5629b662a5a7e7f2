"""LaplaceGP restarts and folds in lock step (models/_laplace_lockstep.py): the batched entry points at their tile edges, searches
of unequal length and with halvings, and the public entry points.  The reference of every assertion is the model's own sequential
path, and every comparison is exact (torch.equal / ==): there are no tolerances in this file."""
import contextlib
import io
import json

import numpy as np
import pytest
import torch

from gptorch_amd import _native, _ops, kernels, likelihoods, mean_functions, rng
from gptorch_amd.models import (GPR, VFE, batched_factorise, batched_log_likelihood, batched_loss_and_grad,
                                multi_start_optimize)
from gptorch_amd.models import _laplace_lockstep as ll
from gptorch_amd.models import _lockstep, laplace
from tests import _laplace_oracle as lo
from tests._util import load_npz

pytestmark = pytest.mark.gpu

GOLD = load_npz("laplace_cases.npz")
CASES = {c["name"]: c for c in json.loads(str(GOLD["meta"]))["cases"]}
LIK_KIND = {"probit": _native.LIK_PROBIT, "logit": _native.LIK_LOGIT, "poisson": _native.LIK_POISSON}
MODE_FIELDS = ("a", "Ka", "f", "value", "d1", "W", "d3", "s", "sum_log_diag")


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def cuda(a):
    return torch.tensor(np.asarray(a, dtype=np.float64)).cuda()


def unif(seed, shape):
    return rng.uniform(seed, int(np.prod(shape))).reshape(shape)


# ---- 1. the batched wrappers against the single ones, per model --------------------------------------------------------------------------
@pytest.mark.parametrize("stacked", [False, True], ids=["shared_x", "stacked_x"])
@pytest.mark.parametrize("d", [1, 17])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 257])
def test_batched_entry_points_equal_the_single_ones(device, n, d, stacked):
    B = 3
    ard = n % 2 == 1
    kind = "Matern52" if d == 1 else "Rbf"
    seed = 5000 + 37 * n + d
    xs = [rng.normal(seed + b, (n, d)) * (1.0 / np.sqrt(d)) for b in range(B)]
    X = cuda(np.stack(xs)) if stacked else cuda(xs[0])
    Xb = lambda b: X[b] if stacked else X
    var = cuda([0.6, 1.3, 2.1])
    ls = cuda(0.7 + 0.6 * unif(seed + 10, (B, d if ard else 1)))
    vec = lambda k: cuda(rng.normal(seed + 20 + k, (B, n)))
    pos = lambda k: cuda(0.05 + 2.0 * unif(seed + 40 + k, (B, n)))

    # gpn_lik_derivs_batched: every likelihood, shared and stacked targets
    f = vec(0)
    for lik, kid in LIK_KIND.items():
        y = np.floor(6.0 * unif(seed + 60, (B, n))) if lik == "poisson" else (unif(seed + 61, (B, n)) < 0.5).astype(np.float64)
        y = cuda(y) if stacked else cuda(y[0])
        got = _ops.lik_derivs_batched(kid, f, y)
        for b in range(B):
            want = _ops.lik_derivs(kid, f[b], y[b] if stacked else y)
            assert all(torch.equal(g[b], w) for g, w in zip(got, want)), (lik, b)
        only = _ops.lik_derivs_batched(kid, f, y, want_d3=False)
        assert only[3] is None and all(torch.equal(g, o) for g, o in zip(got[:3], only[:3]))

    # gpn_laplace_system_batched into sentinel-filled slots: equal to the single call into a sentinel-filled buffer, EVERYWHERE --
    # so nothing outside each slot's lower triangle is touched
    s = pos(0)
    sentinel = -7.25
    fb = _ops.FactorBatch(B, n, 1, device)
    fb.A.fill_(sentinel)
    _ops.laplace_system_batched(kind, X, var, ls, s, fb)
    slots = fb.A.view(B, fb.rows, fb.ld)
    for b in range(B):
        A = torch.full((fb.rows, fb.ld), sentinel, dtype=torch.float64, device=device)
        _ops.laplace_system(kind, Xb(b), var[b:b + 1], ls[b], s[b], A, fb.ld)
        assert torch.equal(slots[b], A), b
        low = torch.tril(torch.ones(n, n, dtype=torch.bool, device=device))
        assert bool((slots[b][:n, :n][~low] == sentinel).all()) and bool((slots[b][:n, n:] == sentinel).all())
        assert bool((slots[b][n:] == sentinel).all()) and not bool((slots[b][:n, :n][low] == sentinel).any())

    # gpn_laplace_matvec_batched
    v = vec(1)
    got = _ops.laplace_matvec_batched(kind, X, var, ls, v)
    for b in range(B):
        assert torch.equal(got[b], _ops.laplace_matvec(kind, Xb(b), var[b:b + 1], ls[b], v[b])), b

    # gpn_laplace_diag_batched / gpn_laplace_grad_batched: every model's Binv at a stride
    rp = _ops.round_up(n, 64)
    g = rng.normal(seed + 70, (B, n, n + 3))
    binv = np.einsum("bik,bjk->bij", g, g) / (n + 3) + 0.5 * np.eye(n)
    Binv = torch.zeros(B, rp, fb.ld, dtype=torch.float64, device=device)
    Binv[:, :n, :n] = cuda(binv)
    got = _ops.laplace_diag_batched(kind, X, var, ls, s, Binv, fb.ld, rp * fb.ld)
    for b in range(B):
        assert torch.equal(got[b], _ops.laplace_diag(kind, Xb(b), var[b:b + 1], ls[b], s[b], Binv[b])), b
    a, u, d1 = vec(2), vec(3), vec(4)
    got = _ops.laplace_grad_batched(kind, X, var, ls, s, Binv, fb.ld, rp * fb.ld, a, u, d1)
    assert got.shape == (B, 1 + ls.shape[1])
    for b in range(B):
        assert torch.equal(got[b], _ops.laplace_grad(kind, Xb(b), var[b:b + 1], ls[b], s[b], Binv[b], a[b], u[b], d1[b])), b

    # gpn_backsub_batched after a lock-step factorisation of an SPD batch with a packed extra row
    fb = _ops.FactorBatch(B, n, 1, device)
    _ops.laplace_system_batched(kind, X, var, ls, s, fb)
    fb.A.view(B, fb.rows, fb.ld)[:, n, :n] = vec(5)
    st = _native.lib().gpn_potrf_lower_batched(_ops._stream(device), _ops._ptr(fb.A), n, 1, fb.ld, fb.sA, _ops._ptr(fb.winv), fb.sW,
                                               _ops._ptr(fb.info), B)
    assert st == 0 and fb.info.tolist() == [0] * B
    got = _ops.backsub_batched(fb)
    assert got.shape == (B, 1, n)
    for b in range(B):
        assert torch.equal(got[b], _ops.backsub(fb.factor(b))), b
    assert torch.equal(_ops.backsub_batched(fb, 2), got[:2])             # a sub-batch in the first slots


# ---- 2. / 3. searches of unequal length, with halvings ---------------------------------------------------------------------------------------
def _search_problem(name, hypers):
    case = CASES[name]
    inp = lo.case_inputs(case)
    base_ls = np.atleast_1d(np.asarray(case["length_scales"], dtype=np.float64))
    oracle = [lo.LaplaceOracle(inp["x"], inp["y"], case["kind"], case["lik"], v, base_ls * fac, ARD=bool(case["ARD"])).search() for v, fac in hypers]
    X, y = cuda(inp["x"]), cuda(inp["y"]).reshape(-1)
    var = cuda([v for v, _ in hypers])
    ls = cuda(np.stack([base_ls * fac for _, fac in hypers]))
    return case, X, y, var, ls, [(o.steps, o.halvings) for o in oracle]


def _assert_modes_equal(got, want):
    for name in MODE_FIELDS:
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert (got.steps, got.halvings) == (want.steps, want.halvings)


def _searches_match(name, hypers, stacked):
    case, X, y, var, ls, oracle = _search_problem(name, hypers)
    B, n = len(hypers), X.shape[0]
    kind, lik = case["kind"], LIK_KIND[case["lik"]]
    m = torch.zeros(n, dtype=torch.float64, device=X.device)
    want = [laplace.find_mode(kind, lik, X, y, m, var[b:b + 1], ls[b]) for b in range(B)]
    before = dict(ll.STATS)
    Xs, ys = (torch.stack([X] * B), torch.stack([y] * B)) if stacked else (X, y)
    got = ll.find_modes(kind, lik, Xs, ys, torch.zeros(B, n, dtype=torch.float64, device=X.device), var, ls, [None] * B, [1e-8] * B, [50] * B)
    stats = {k: ll.STATS[k] - before[k] for k in before}
    for g, w in zip(got, want):
        _assert_modes_equal(g, w)
    steps = [w.steps for w in want]
    print("%s: oracle (steps, halvings) %s, find_mode %s, STATS %s" % (name, oracle, [(w.steps, w.halvings) for w in want], stats))
    assert stats["searches"] == 1 and stats["rounds"] == max(steps)
    assert stats["factorisations"] == sum(steps) + B                     # converged models were not factorised again
    assert stats["trial_reads"] >= stats["rounds"]
    return oracle, want, got


@pytest.mark.parametrize("stacked", [False, True], ids=["shared_x", "stacked_x"])
def test_searches_of_unequal_length(device, stacked):
    oracle, want, _ = _searches_match("probit_rbf_300x2", [(0.3, 1.0), (1.7, 1.0), (8.0, 0.5)], stacked)
    assert len({s for s, _ in oracle}) > 1, oracle                       # the case has not degenerated: the searches differ in length
    assert len({w.steps for w in want}) > 1


def test_searches_with_halvings(device):
    oracle, want, _ = _searches_match("poisson_rbf_513x2", [(0.3, 1.0), (4.0, 0.6), (0.05, 2.0)], False)
    assert len({h for _, h in oracle}) > 1 and min(h for _, h in oracle) > 0, oracle
    assert len({w.halvings for w in want}) > 1 and min(w.halvings for w in want) > 0


# ---- the public entry points -------------------------------------------------------------------------------------------------------------
def _restarts(name, hypers, mean=None, shared=True):
    """one LaplaceGP per (variance, length-scale factor) on the case's data (shared: every model holds the first one's tensors)"""
    case = CASES[name]
    inp = lo.case_inputs(case)
    base_ls = np.atleast_1d(np.asarray(case["length_scales"], dtype=np.float64))
    out = []
    for v, fac in hypers:
        mdl = lo.build_model(dict(case, variance=v, length_scales=base_ls * fac, mean=mean), inp)
        mdl.cuda()
        out.append(mdl)
    if shared:
        for mdl in out[1:]:
            mdl.X, mdl.Y = out[0].X, out[0].Y
    return out


def _evaluate_alone(ms):
    out = []
    for mdl in ms:
        mdl.zero_grad()
        loss = mdl.loss()
        loss.backward()
        out.append(loss.detach().clone())
    return out


def _assert_same_state(got_losses, lock, want_losses, alone):
    for l1, mb, l0, ma in zip(got_losses, lock, want_losses, alone):
        assert l0.shape == l1.shape and torch.equal(l0, l1), (l0.item(), l1.item())
        for p, q in zip(ma.parameters(), mb.parameters()):
            assert (p.grad is None) == (q.grad is None)
            if p.grad is not None:
                assert p.grad.shape == q.grad.shape and torch.equal(p.grad, q.grad), (p.grad, q.grad)
        assert torch.equal(ma._mode_a, mb._mode_a) and ma.newton_stats == mb.newton_stats


@pytest.mark.parametrize("with_mean", [False, True], ids=["zero_mean", "constant_mean_and_prior"])
def test_batched_loss_and_grad(device, with_mean):
    """three cold restarts and one warm-started model (primed by one own loss() at variance x 1.05), then everything warm.  (The
    copies evaluated alone are built a second time from the same inputs: copy.deepcopy of a Param drops its transform.)"""
    hypers = [(0.3, 1.0), (1.7, 1.0), (8.0, 0.5), (1.1, 0.8)]

    def fresh():
        ms = _restarts("probit_rbf_300x2", hypers, mean=0.2 if with_mean else None)
        primer = _restarts("probit_rbf_300x2", [(1.1 * 1.05, 0.8)], mean=0.2 if with_mean else None)[0]
        primer.X, primer.Y = ms[0].X, ms[0].Y
        primer.loss()
        primer.kernel.variance.data.copy_(ms[3].kernel.variance.data)     # the warm model: the fourth one's parameters, the primer's mode
        ms[3] = primer
        if with_mean:
            ms[1].kernel.variance.prior = torch.distributions.Gamma(torch.tensor(2.0, dtype=torch.float64, device=device),
                                                                    torch.tensor(1.0, dtype=torch.float64, device=device))
        return ms
    lock, alone = fresh(), fresh()
    assert lock[3]._mode_a is not None and all(m._mode_a is None for m in lock[:3])
    assert len(_lockstep._laplace_groups(lock)) == 1
    for _call in range(2):
        want = _evaluate_alone(alone)
        for mdl in lock:
            mdl.zero_grad()
        before = ll.STATS["searches"]
        got = batched_loss_and_grad(lock)
        assert ll.STATS["searches"] == before + 1                         # the lock-step path ran
        _assert_same_state(got, lock, want, alone)
    if with_mean:
        means = list(lock[0].mean_function.parameters())
        assert means and all(p.grad is not None for p in means)
        assert got[1].item() != (-(lock[1].log_likelihood())).item()      # the prior really is in the loss
    values = batched_log_likelihood(lock)
    for v, mdl in zip(values, alone):
        own = mdl.log_likelihood().detach()
        assert v.shape == own.shape and torch.equal(v, own)


def test_multi_start_optimize(device):
    hypers = [(0.3, 1.0), (1.7, 1.0), (8.0, 0.5)]
    lock, alone = _restarts("probit_rbf_300x2", hypers), _restarts("probit_rbf_300x2", hypers)
    with quiet():
        before = ll.STATS["searches"]
        losses, _ = multi_start_optimize(lock, method="Adam", max_iter=5)
        assert ll.STATS["searches"] == before + 5
        own = [np.asarray(mdl.optimize(method="Adam", max_iter=5)[0], dtype=np.float64).reshape(-1) for mdl in alone]
    for b in range(3):
        assert np.array_equal(losses[b], own[b]), (losses[b], own[b])
        for p, q in zip(alone[b].parameters(), lock[b].parameters()):
            assert torch.equal(p.data, q.data)
    lock, alone = _restarts("probit_rbf_300x2", hypers[:2]), _restarts("probit_rbf_300x2", hypers[:2])
    with quiet():
        before = ll.STATS["searches"]
        res, _ = multi_start_optimize(lock, method="L-BFGS-B", max_iter=5)
        assert ll.STATS["searches"] > before
        own = [mdl.optimize(method="L-BFGS-B", max_iter=5) for mdl in alone]
    for r0, r1 in zip(own, res):
        assert np.array_equal(r0.x, r1.x) and r0.fun == r1.fun and r0.nfev == r1.nfev


def test_batched_factorise_seeds_the_predictions(device, monkeypatch):
    """three fitted folds of equal length (every model its own rows): the predictions of the seeded models equal those of copies
    that predicted alone, and no seeded model searches again"""
    case = CASES["probit_rbf_300x2"]
    inp = lo.case_inputs(case)

    def fresh():
        folds = []
        for b, (v, fac) in enumerate([(0.9, 1.0), (1.7, 0.8), (2.6, 1.2)]):
            keep = np.ones(300, dtype=bool)
            keep[b * 100:(b + 1) * 100] = False
            mdl = lo.build_model(dict(case, variance=v, length_scales=np.atleast_1d(case["length_scales"]) * fac),
                                 {"x": inp["x"][keep], "y": inp["y"][keep]})
            mdl.cuda()
            folds.append(mdl)
        return folds
    folds, alone = fresh(), fresh()
    xs = cuda(inp["xs"])
    want = [(mdl.predict_f(xs), mdl.predict_y(xs)) for mdl in alone]
    assert batched_factorise(folds) == 3

    def no_search(*args, **kwargs):
        raise AssertionError("a seeded model searched again")
    monkeypatch.setattr(laplace, "find_mode", no_search)
    for mdl, ref, (wf, wy) in zip(folds, alone, want):
        gf, gy = mdl.predict_f(xs), mdl.predict_y(xs)
        assert all(torch.equal(g, w) for g, w in zip(list(gf) + list(gy), list(wf) + list(wy)))
        assert mdl._predict_calls == ref._predict_calls == 2              # two lookups served by one state, in both
        assert torch.equal(mdl._mode_a, ref._mode_a) and mdl.newton_stats == ref.newton_stats


def test_a_model_that_does_not_converge_falls_out(device):
    hypers = [(0.3, 1.0), (1.7, 1.0), (8.0, 0.5)]
    lock, alone = _restarts("probit_rbf_300x2", hypers), _restarts("probit_rbf_300x2", hypers)
    lock[1].max_newton_iter = alone[1].max_newton_iter = 1
    with pytest.raises(RuntimeError) as own:
        alone[1].loss()
    with pytest.raises(RuntimeError) as got:
        batched_loss_and_grad(lock)
    assert str(got.value) == str(own.value) and "did not converge in 1 Newton steps" in str(got.value)
    assert all(m._mode_a is None for m in lock)                           # nobody's state moved
    rest, rest_alone = [lock[0], lock[2]], [alone[0], alone[2]]
    want = _evaluate_alone(rest_alone)
    for mdl in rest:
        mdl.zero_grad()
    _assert_same_state(batched_loss_and_grad(rest), rest, want, rest_alone)


def test_a_replay_that_returns_is_a_disagreement(device, monkeypatch):
    """a model that fails in the group is replayed alone to raise its own error; a replay that RETURNS (here: a stand-in for
    find_mode) means the two searches disagree, and the call raises that -- nobody's state moved"""
    lock = _restarts("probit_rbf_300x2", [(0.3, 1.0), (1.7, 1.0), (8.0, 0.5)])
    lock[1].max_newton_iter = 1
    monkeypatch.setattr(laplace, "find_mode", lambda *args, **kwargs: object())
    with pytest.raises(_native.NativeError, match="disagree") as got:
        batched_loss_and_grad(lock)
    assert "LaplaceGP: model 1 " in str(got.value)
    assert all(m._mode_a is None for m in lock)


def test_backward_survives_a_later_forward(device):
    """the group's factor slots are reused by the next forward: an earlier node rebuilds its factors privately (the `generation`
    check), and its gradients are those taken immediately"""
    lock = _restarts("probit_rbf_300x2", [(0.3, 1.0), (1.7, 1.0), (8.0, 0.5)], mean=0.2)
    (key, g), = _lockstep._laplace_groups(lock)
    group = _lockstep.Group(None, key, g)

    def forward():
        for mdl in lock:
            mdl.reset_mode()
            mdl.zero_grad()
        return -_lockstep._laplace_group_evidence(lock, group, differentiable=True)

    def grads():
        return [p.grad.clone() for mdl in lock for p in mdl.parameters() if p.grad is not None]
    first = forward()
    first.sum().backward()
    want = grads()
    assert len(want) == 9
    first = forward()
    with torch.no_grad():
        for mdl in lock:
            mdl.kernel.variance.data += 0.1
    for mdl in lock:
        mdl.reset_mode()
    later = -_lockstep._laplace_group_evidence(lock, group, differentiable=True)  # refactorises the shared slots at other parameters
    assert not torch.equal(later.detach(), first.detach())
    with torch.no_grad():
        for mdl in lock:
            mdl.kernel.variance.data -= 0.1
    factorised = ll.STATS["factorisations"]
    first.sum().backward()
    assert ll.STATS["factorisations"] == factorised + 3                   # the private rebuild happened
    assert all(torch.equal(a, b) for a, b in zip(grads(), want))


def test_mixed_list(device):
    """GPR + VFE + LaplaceGP groups and a singleton LaplaceGP of another N in one call"""
    def build():
        x, y = rng.make_regression(256, 2, 1, seed=3)
        g = [GPR(x, y, kernels.Rbf(2, variance=1.0 + 0.1 * i)) for i in range(2)]
        v = [VFE(x, y, kernels.Rbf(2, variance=0.8 + 0.2 * i), inducing_points=x[:24] + 0.01 * i, likelihood=likelihoods.Gaussian(variance=0.05),
                 mean_function=mean_functions.Zero(1)) for i in range(2)]
        for mdl in g + v:
            mdl.cuda()
        lap = _restarts("probit_rbf_300x2", [(0.3, 1.0), (1.7, 1.0)])
        lone = _restarts("poisson_rbf_513x2", [(0.3, 1.0)])
        return [lap[0], g[0], v[0], lone[0], lap[1], g[1], v[1]]
    lock, alone = build(), build()
    plan = _lockstep._plan_groups(lock)
    assert [grp.family.name for grp in plan] == ["lml", "vfe", "laplace"] and plan[-1].indices == [0, 4]
    want = _evaluate_alone(alone)
    for mdl in lock:
        mdl.zero_grad()
    got = batched_loss_and_grad(lock)
    for l0, l1, ma, mb in zip(want, got, alone, lock):
        assert l0.shape == l1.shape and torch.equal(l0, l1)
        for p, q in zip(ma.parameters(), mb.parameters()):
            assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad))
