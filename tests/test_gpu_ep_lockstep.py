"""EPGP restarts and folds in lock step (models/_ep_lockstep.py): gpn_ep_sites_batched at its tile edges, searches of unequal
length, per-model settings, the stall rule, a model that falls out, and the public entry points.  The reference of every assertion
but the last test's is the model's own sequential path, and every such comparison is exact (torch.equal / ==); the last test anchors
the lock-step numbers directly to the goldens with the tolerances of tests/test_gpu_ep.py::test_model_case."""
import contextlib
import io
import json

import numpy as np
import pytest
import torch

from gptorch_amd import _native, _ops, kernels, likelihoods, rng
from gptorch_amd.models import GPR, batched_factorise, batched_log_likelihood, batched_loss_and_grad, multi_start_optimize
from gptorch_amd.models import _ep_lockstep as el
from gptorch_amd.models import _laplace_lockstep as ll
from gptorch_amd.models import _lockstep, ep
from tests import _ep_oracle as eo
from tests import _laplace_oracle as lo
from tests import _xref as xr
from tests._util import load_npz

pytestmark = pytest.mark.gpu

GOLD = load_npz("ep_cases.npz")
META = json.loads(str(GOLD["meta"]))
CASES = {c["name"]: c for c in META["cases"]}
LAPLACE_CASES = {c["name"]: c for c in json.loads(str(load_npz("laplace_cases.npz")["meta"]))["cases"]}
LIK_KIND = {"probit": _native.LIK_PROBIT, "logit": _native.LIK_LOGIT}
SITE_FIELDS = ("tau", "nu", "a", "Ka", "s", "mu", "sigma2", "mu_hat", "s2_hat", "evidence")
SETTINGS = [(0.3, 1.0), (1.7, 1.0), (8.0, 0.5)]         # (variance, length-scale): tests/test_ep_lockstep_host.py checks, on the CPU
#                                                          oracle, that their searches differ in length


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def cuda(a):
    return torch.tensor(np.asarray(a, dtype=np.float64)).cuda()


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and torch.equal(a, b))


# ---- 1. gpn_ep_sites_batched against gpn_ep_sites, per row -------------------------------------------------------------------------------
@pytest.mark.parametrize("link", ["probit", "logit2", "logit20", "logit64"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513, 65537])
def test_ep_sites_batched_equals_the_single_call_per_row(device, n, link):
    B = 3
    lik = link[:6] if link.startswith("probit") else "logit"
    rule = likelihoods.gauss_hermite(int(link[5:]), device) if lik == "logit" else (None, None)
    npts = GOLD["pw_%s_mu" % lik].size
    # the golden points dealt over the rows as test_ep_sites_match_the_goldens deals them, a different offset per model
    idx = np.stack([(np.arange(n) * 7 + n + 1013 * b) % npts for b in range(B)])
    Y, M, mu, sigma2, tau, nu = (cuda(GOLD["pw_%s_%s" % (lik, k)][idx]) for k in ("y", "m", "mu", "sigma2", "tau", "nu"))
    rho = [0.5, 0.8, 1.0]
    rho_dev = cuda(rho)
    for stacked_y in (False, True):
        for with_m in (False, True):
            for moments_only in (False, True):
                y, m = (Y if stacked_y else Y[0]), (M if with_m else None)

                def run(count=B, want_moments=True):
                    return _ops.ep_sites_batched(LIK_KIND[lik], y[:count] if stacked_y else y, None if m is None else m[:count], mu[:count],
                                                 sigma2[:count], tau[:count], nu[:count], rho_dev[:count], *rule, moments_only=moments_only,
                                                 want_moments=want_moments)
                got = run()
                assert got[5].shape == (B, 6) and (got[0] is None) == moments_only and (got[1] is None) == moments_only
                for b in range(B):
                    want = _ops.ep_sites(LIK_KIND[lik], Y[b] if stacked_y else Y[0], None if m is None else M[b], mu[b], sigma2[b], tau[b],
                                         nu[b], rho[b], *rule, moments_only=moments_only)
                    for k, (g, w) in enumerate(zip(got, want)):
                        assert same(None if g is None else g[b], w), (stacked_y, with_m, moments_only, b, k)
                assert all(same(a, b) for a, b in zip(got, run()))                          # the same call twice: the same bits
                bare = run(want_moments=False)                                              # null moment outputs: the rest unchanged
                assert bare[2] is None and bare[3] is None and bare[4] is None
                assert same(bare[0], got[0]) and same(bare[1], got[1]) and same(bare[5], got[5])
                sub = run(count=2)                                                          # a sub-batch of 2 in the 3-slot allocation
                assert all(same(s, None if g is None else g[:2]) for s, g in zip(sub, got))


# ---- 2. searches of unequal length ---------------------------------------------------------------------------------------------------------
def _assert_sites_equal(got, want):
    for name in SITE_FIELDS:
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape and torch.equal(g, w), name
    assert (got.sweeps, got.stalled) == (want.sweeps, want.stalled)


@pytest.mark.parametrize("stacked", [False, True], ids=["shared_x", "stacked_x"])
@pytest.mark.parametrize("name", ["probit_rbf_300x2", "logit_matern52_300x3"])
def test_searches_of_unequal_length(device, name, stacked):
    case = CASES[name]
    inp = lo.case_inputs(case)
    B = len(SETTINGS)
    X, y = cuda(inp["x"]), cuda(inp["y"]).reshape(-1)
    n = X.shape[0]
    kind, lik = case["kind"], LIK_KIND[case["lik"]]
    rule = likelihoods.gauss_hermite(int(case["H"]), device) if case["lik"] == "logit" else (None, None)
    var, ls = cuda([v for v, _ in SETTINGS]), cuda([[ell] for _, ell in SETTINGS])
    m = torch.full((n,), 0.0 if case["mean"] is None else float(case["mean"]), dtype=torch.float64, device=device)
    want = [ep.find_sites(kind, lik, X, y, m, var[b:b + 1], ls[b], rule=rule) for b in range(B)]
    Xs, ys = (torch.stack([X] * B), torch.stack([y] * B)) if stacked else (X, y)
    before = dict(el.STATS)
    laplace_before = dict(ll.STATS)
    got = el.find_sites_batched(kind, lik, Xs, ys, torch.stack([m] * B), var, ls, rule, [None] * B, [1e-10] * B, [200] * B, [0.8] * B)
    stats = {k: el.STATS[k] - before[k] for k in before}
    for g, w in zip(got, want):
        _assert_sites_equal(g, w)
    sweeps = [w.sweeps for w in want]
    print("%s: find_sites sweeps %s, STATS %s" % (name, sweeps, stats))
    assert len(set(sweeps)) > 1                                           # the searches differ in length: models left one by one
    assert stats == {"searches": 1, "sweeps": max(sweeps), "reads": max(sweeps), "factorisations": sum(sweeps) + B}
    assert ll.STATS == laplace_before                                     # (LaplaceGP's counters are its own)


# ---- the public entry points ---------------------------------------------------------------------------------------------------------------
def _restarts(name, settings, mean="case", shared=True):
    """one EPGP per (variance, length-scale) on the case's data (shared: every model holds the first one's tensors)"""
    case = CASES[name]
    inp = lo.case_inputs(case)
    out = []
    for v, ell in settings:
        mdl = eo.build_model(dict(case, variance=v, length_scales=[ell], mean=case["mean"] if mean == "case" else mean), inp)
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
        assert all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(ma._sites, mb._sites)) and ma.ep_stats == mb.ep_stats


def _lock_step(lock):
    for mdl in lock:
        mdl.zero_grad()
    before = el.STATS["searches"]
    got = batched_loss_and_grad(lock)
    assert el.STATS["searches"] == before + 1                             # the lock-step path ran
    return got


# ---- 3. per-model settings -----------------------------------------------------------------------------------------------------------------
def test_per_model_settings(device):
    """one group whose models differ in damping, ep_tol and start: the fourth model is warm (primed by one own loss() at
    variance x 1.05), the others cold; then everything once more, all warm"""
    settings = SETTINGS + [(1.1, 0.8)]

    def fresh():
        ms = _restarts("probit_rbf_300x2", settings)
        primer = _restarts("probit_rbf_300x2", [(1.1 * 1.05, 0.8)])[0]
        primer.X, primer.Y = ms[0].X, ms[0].Y
        primer.loss()
        primer.kernel.variance.data.copy_(ms[3].kernel.variance.data)     # the warm model: the fourth one's parameters, the primer's sites
        ms[3] = primer
        ms[0].damping, ms[1].damping, ms[2].damping, ms[3].damping = 0.5, 0.8, 0.5, 0.8
        ms[0].ep_tol, ms[1].ep_tol, ms[2].ep_tol, ms[3].ep_tol = 1e-10, 1e-6, 1e-6, 1e-10
        return ms
    lock, alone = fresh(), fresh()
    assert lock[3]._sites is not None and all(m._sites is None for m in lock[:3])
    assert len(_lockstep._ep_groups(lock)) == 1
    for call in range(2):
        want = _evaluate_alone(alone)
        _assert_same_state(_lock_step(lock), lock, want, alone)
        print("per-model settings: ep_stats %s" % [m.ep_stats for m in lock])
        # the first call's searches differ in length (the second call finds everyone at its sites)
        assert call == 1 or len({m.ep_stats["sweeps"] for m in lock}) > 1


# ---- 4. a search that ends by the stall rule -----------------------------------------------------------------------------------------------
def test_a_search_that_stalls(device):
    """ep_tol = 0 for the second model (tests/test_ep_lockstep_host.py: the CPU oracle ends that search by the stall rule)"""
    lock, alone = _restarts("probit_rbf_300x2", SETTINGS), _restarts("probit_rbf_300x2", SETTINGS)
    lock[1].ep_tol = alone[1].ep_tol = 0.0
    want = _evaluate_alone(alone)
    _assert_same_state(_lock_step(lock), lock, want, alone)
    print("stall: ep_stats %s" % [m.ep_stats for m in lock])
    assert lock[1].ep_stats["stalled"] and not lock[0].ep_stats["stalled"] and not lock[2].ep_stats["stalled"]
    # the others are what they are in a group without the stalling model
    rest, rest_alone = _restarts("probit_rbf_300x2", [SETTINGS[0], SETTINGS[2]]), [alone[0], alone[2]]
    _assert_same_state(_lock_step(rest), rest, [want[0], want[2]], rest_alone)


# ---- 5. a model that falls out -------------------------------------------------------------------------------------------------------------
def test_a_model_that_does_not_converge_falls_out(device):
    lock, alone = _restarts("probit_rbf_300x2", SETTINGS), _restarts("probit_rbf_300x2", SETTINGS)
    lock[1].max_sweeps = alone[1].max_sweeps = 2
    with pytest.raises(RuntimeError) as own:
        alone[1].loss()
    with pytest.raises(RuntimeError) as got:
        batched_loss_and_grad(lock)
    assert str(got.value) == str(own.value) and "did not converge in 2 sweeps" in str(got.value)
    assert all(m._sites is None for m in lock)                            # nobody's state moved
    rest, rest_alone = [lock[0], lock[2]], [alone[0], alone[2]]
    want = _evaluate_alone(rest_alone)
    _assert_same_state(_lock_step(rest), rest, want, rest_alone)


def test_a_replay_that_returns_is_a_disagreement(device, monkeypatch):
    """a model that fails in the group is replayed alone to raise its own error; a replay that RETURNS (here: a stand-in for
    find_sites) means the two searches disagree, and the call raises that -- nobody's state moved"""
    lock = _restarts("probit_rbf_300x2", SETTINGS)
    lock[1].max_sweeps = 1
    monkeypatch.setattr(ep, "find_sites", lambda *args, **kwargs: object())
    with pytest.raises(_native.NativeError, match="disagree") as got:
        batched_loss_and_grad(lock)
    assert "EPGP: model 1 " in str(got.value)
    assert all(m._sites is None for m in lock)


# ---- 6. batched_log_likelihood and batched_loss_and_grad -----------------------------------------------------------------------------------
@pytest.mark.parametrize("with_mean", [False, True], ids=["zero_mean", "constant_mean_and_prior"])
def test_batched_loss_and_grad(device, with_mean):
    def fresh():
        ms = _restarts("probit_rbf_300x2", SETTINGS, mean=0.2 if with_mean else None)
        if with_mean:
            ms[1].kernel.variance.prior = torch.distributions.Gamma(torch.tensor(2.0, dtype=torch.float64, device=device),
                                                                    torch.tensor(1.0, dtype=torch.float64, device=device))
        return ms
    lock, alone = fresh(), fresh()
    for _call in range(2):                                                # cold, then warm
        want = _evaluate_alone(alone)
        got = _lock_step(lock)
        _assert_same_state(got, lock, want, alone)
    if with_mean:
        means = list(lock[0].mean_function.parameters())
        assert means and all(p.grad is not None for p in means)
    before = el.STATS["searches"]
    values = batched_log_likelihood(lock)
    assert el.STATS["searches"] == before + 1
    for v, mdl, mb in zip(values, alone, lock):
        own = mdl.log_likelihood().detach()
        assert v.shape == own.shape and torch.equal(v, own)
        assert all(torch.equal(a, b) for a, b in zip(mdl._sites, mb._sites)) and mdl.ep_stats == mb.ep_stats
    if with_mean:
        # the prior really is in the loss (log p(1.7) under Gamma(2, 1) is -1.17; a warm re-evaluation moves the evidence by ~1e-10)
        assert abs(got[1].item() + values[1].item()) > 0.1 and abs(got[0].item() + values[0].item()) < 1e-6


# ---- 7. multi_start_optimize ---------------------------------------------------------------------------------------------------------------
def test_multi_start_optimize(device):
    lock, alone = _restarts("probit_rbf_300x2", SETTINGS), _restarts("probit_rbf_300x2", SETTINGS)
    with quiet():
        before = el.STATS["searches"]
        losses, _ = multi_start_optimize(lock, method="Adam", max_iter=3)
        assert el.STATS["searches"] == before + 3
        own = [np.asarray(mdl.optimize(method="Adam", max_iter=3)[0], dtype=np.float64).reshape(-1) for mdl in alone]
    for b in range(3):
        assert np.array_equal(losses[b], own[b]), (losses[b], own[b])
        for p, q in zip(alone[b].parameters(), lock[b].parameters()):
            assert torch.equal(p.data, q.data)
    lock, alone = _restarts("probit_rbf_300x2", SETTINGS[:2]), _restarts("probit_rbf_300x2", SETTINGS[:2])
    with quiet():
        before = el.STATS["searches"]
        res, _ = multi_start_optimize(lock, method="L-BFGS-B", max_iter=3)
        assert el.STATS["searches"] > before
        own = [mdl.optimize(method="L-BFGS-B", max_iter=3) for mdl in alone]
    for r0, r1 in zip(own, res):
        assert np.array_equal(r0.x, r1.x) and r0.fun == r1.fun and r0.nfev == r1.nfev
    # capture=True: EPGP models keep their own optimize() (the search reads the host)
    lock = _restarts("probit_rbf_300x2", SETTINGS[:2])
    with quiet():
        before = el.STATS["searches"]
        multi_start_optimize(lock, method="Adam", max_iter=1, capture=True)
    assert el.STATS["searches"] == before


# ---- 8. batched_factorise ------------------------------------------------------------------------------------------------------------------
def test_batched_factorise_seeds_the_predictions(device, monkeypatch):
    """three fitted folds of equal length (every model its own rows): the predictions of the seeded models equal those of copies
    that predicted alone, and no seeded model searches again"""
    case = CASES["probit_rbf_300x2"]
    inp = lo.case_inputs(case)

    def fresh():
        folds = []
        for b, (v, ell) in enumerate([(0.9, 0.9), (1.7, 0.7), (2.6, 1.1)]):
            keep = np.ones(300, dtype=bool)
            keep[b * 100:(b + 1) * 100] = False
            mdl = eo.build_model(dict(case, variance=v, length_scales=[ell]), {"x": inp["x"][keep], "y": inp["y"][keep]})
            mdl.cuda()
            folds.append(mdl)
        return folds
    folds, alone = fresh(), fresh()
    xs = cuda(inp["xs"])
    want = [(mdl.predict_f(xs), mdl.predict_y(xs)) for mdl in alone]
    assert batched_factorise(folds) == 3
    after = dict(el.STATS)

    def no_search(*args, **kwargs):
        raise AssertionError("a seeded model searched again")
    monkeypatch.setattr(ep, "find_sites", no_search)
    for mdl, ref, (wf, wy) in zip(folds, alone, want):
        gf, gy = mdl.predict_f(xs), mdl.predict_y(xs)
        assert all(torch.equal(g, w) for g, w in zip(list(gf) + list(gy), list(wf) + list(wy)))
        assert mdl._predict_calls == ref._predict_calls == 2              # two lookups served by one state, in both
        assert all(torch.equal(a, b) for a, b in zip(mdl._sites, ref._sites)) and mdl.ep_stats == ref.ep_stats
    assert el.STATS == after                                              # ... and no lock-step search either


# ---- 9. a mixed list -----------------------------------------------------------------------------------------------------------------------
def test_mixed_list(device):
    """GPR, LaplaceGP, EPGP probit, EPGP logit H = 20 and EPGP logit H = 32 in one call: five groups, each its own way"""
    def build():
        x, y = rng.make_regression(256, 2, 1, seed=3)
        g = [GPR(x, y, kernels.Rbf(2, variance=1.0 + 0.1 * i)) for i in range(2)]
        lcase = LAPLACE_CASES["probit_rbf_300x2"]
        linp = lo.case_inputs(lcase)
        lap = [lo.build_model(dict(lcase, variance=v), linp) for v in (0.3, 1.7)]
        for mdl in g + lap:
            mdl.cuda()
        probit = _restarts("probit_rbf_300x2", SETTINGS[:2])
        h32 = _restarts("logit_matern52_300x3", SETTINGS[:2])
        h20 = _restarts("logit_matern52_300x3", SETTINGS[:2])
        for mdl in h20:
            mdl.likelihood.num_gauss_hermite_points = 20
        return [probit[0], g[0], lap[0], h20[0], h32[0], probit[1], g[1], lap[1], h20[1], h32[1]]
    lock, alone = build(), build()
    plan = _lockstep._plan_groups(lock)
    assert [grp.family.name for grp in plan] == ["lml", "laplace", "ep", "ep", "ep"]
    assert sorted((grp.family.name, getattr(grp.key, "H", None), grp.indices) for grp in plan[1:]) == \
        [("ep", 0, [0, 5]), ("ep", 20, [3, 8]), ("ep", 32, [4, 9]), ("laplace", None, [2, 7])]
    want = _evaluate_alone(alone)
    for mdl in lock:
        mdl.zero_grad()
    before, laplace_before = el.STATS["searches"], ll.STATS["searches"]
    got = batched_loss_and_grad(lock)
    assert el.STATS["searches"] == before + 3 and ll.STATS["searches"] == laplace_before + 1
    for l0, l1, ma, mb in zip(want, got, alone, lock):
        assert l0.shape == l1.shape and torch.equal(l0, l1)
        for p, q in zip(ma.parameters(), mb.parameters()):
            assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad))
    assert want[3].item() != want[4].item()                               # H is part of a logit model's definition


# ---- 10. backward after a later forward ----------------------------------------------------------------------------------------------------
def test_backward_survives_a_later_forward(device):
    """the group's factor slots are reused by the next forward: an earlier node rebuilds its factors privately (the `generation`
    check), and its gradients are those taken immediately"""
    lock = _restarts("probit_rbf_300x2", SETTINGS, mean=0.2)
    (key, g), = _lockstep._ep_groups(lock)
    group = _lockstep.Group(None, key, g)

    def forward():
        for mdl in lock:
            mdl.reset_sites()
            mdl.zero_grad()
        return -_lockstep._ep_group_evidence(lock, group, differentiable=True)

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
        mdl.reset_sites()
    later = -_lockstep._ep_group_evidence(lock, group, differentiable=True)  # refactorises the shared slots at other parameters
    assert not torch.equal(later.detach(), first.detach())
    with torch.no_grad():
        for mdl in lock:
            mdl.kernel.variance.data -= 0.1
    factorised = el.STATS["factorisations"]
    first.sum().backward()
    assert el.STATS["factorisations"] == factorised + 3                   # the private rebuild happened
    assert all(torch.equal(a, b) for a, b in zip(grads(), want))


# ---- 11. the lock-step numbers against the goldens -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_golden_case_as_a_group_of_two(device, name):
    """the evidence and gradients of B = 2 copies of a golden case, taken in lock step, within the tolerances of test_model_case"""
    case = CASES[name]
    e = case["e64"]
    inp = lo.case_inputs(case)
    lock = [eo.build_model(case, inp) for _ in range(2)]
    for mdl in lock:
        mdl.cuda()
    got = _lock_step(lock)
    for b, mdl in enumerate(lock):
        err = xr.rel_err(got[b].item(), case["loss"])
        print("%s[%d]: loss %.12f golden %.12f rel err %.2e (tol %.1e), %s" % (name, b, got[b].item(), case["loss"], err,
                                                                             xr.tol(e["loss"], "loss"), mdl.ep_stats))
        assert err <= xr.tol(e["loss"], "loss")
        assert not mdl.ep_stats["stalled"] and abs(mdl.ep_stats["sweeps"] - case["sweeps"]) <= 1
        grads = [("variance", mdl.kernel.variance), ("length_scales", mdl.kernel.length_scales)]
        if case["mean"] is not None:
            grads.append(("mean", mdl.mean_function.val))
        for gname, p in grads:
            want = GOLD["%s__grad_%s" % (name, gname)]
            gerr = xr.rel_err(p.grad.cpu().numpy().reshape(want.shape), want)
            print("   d/d%-14s rel err %.2e (tol %.1e)" % (gname, gerr, xr.tol(e["grad"], "grad")))
            assert gerr <= xr.tol(e["grad"], "grad"), gname
