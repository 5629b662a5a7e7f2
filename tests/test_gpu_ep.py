"""EPGP on the GPU: gpn_ep_sites against the pointwise goldens of tests/golden/make_ep_golden.py, and every golden model case
through model.cuda().

Tolerances.  Model quantities: tests/_xref.tol = max(16 e64, FLOOR[what]) with e64 the distance of the oracle's plain-fp64
statement from its long-double one (stored by the maker; never measured against the code under test); loss and gradients
relative to max(1, |reference|) (xr.rel_err), predictions absolute.  Pointwise quantities: max(16 e64, 64 * 2^-53 |golden|) per
entry."""
import contextlib
import io
import json

import numpy as np
import pytest
import torch

from gptorch_amd import _native, _ops, likelihoods
from gptorch_amd.models import _lockstep, multi_start_optimize
from tests import _ep_oracle as eo
from tests import _laplace_oracle as lo
from tests import _xref as xr
from tests._util import load_npz

pytestmark = pytest.mark.gpu

GOLD = load_npz("ep_cases.npz")
META = json.loads(str(GOLD["meta"]))
CASES = {c["name"]: c for c in META["cases"]}
U = 2.0 ** -53
LIK_KIND = {"probit": _native.LIK_PROBIT, "logit": _native.LIK_LOGIT}
# the kernel's outputs by their golden names; the statistics by the golden arrays they reduce
OUTPUTS = ("tau_new", "nu_new", "lz", "mu_hat", "s2_hat")
STAT_SUMS = ((0, "lz"), (1, "site"))
STAT_MAXIMA = ((2, "dtau"), (3, "dnu"))


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def cuda(a):
    return torch.tensor(np.asarray(a, dtype=np.float64)).cuda()


def entry_tol(lik, key, idx):
    return np.maximum(16.0 * GOLD["pw_%s_%s_e64" % (lik, key)][idx], 64.0 * U * np.abs(GOLD["pw_%s_%s" % (lik, key)][idx]))


# ---- gpn_ep_sites -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moments_only", [False, True])
@pytest.mark.parametrize("lik", ["probit", "logit"])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257, 513, 1000])
def test_ep_sites_match_the_goldens(device, lik, rows, moments_only):
    npts = GOLD["pw_%s_mu" % lik].size
    idx = (np.arange(rows) * 7 + rows) % npts                         # the golden points, dealt over the rows
    y, m, mu, sigma2, tau, nu = (cuda(GOLD["pw_%s_%s" % (lik, k)][idx]) for k in ("y", "m", "mu", "sigma2", "tau", "nu"))
    rule = likelihoods.gauss_hermite(META["grid_H"], device) if lik == "logit" else (None, None)

    def run():
        return _ops.ep_sites(LIK_KIND[lik], y, m, mu, sigma2, tau, nu, META["damping"], *rule, moments_only=moments_only)

    got = run()
    assert (got[0] is None and got[1] is None) if moments_only else (got[0] is not None and got[1] is not None)
    for key, g in zip(OUTPUTS, got[:5]):
        if g is None:
            continue
        gold, tol = GOLD["pw_%s_%s" % (lik, key)][idx], entry_tol(lik, key, idx)
        err = np.abs(g.cpu().numpy() - gold)
        print("%s rows %d %s: worst err / tol %.3f" % (lik, rows, key, np.max(err / np.maximum(tol, 1e-300))))
        assert np.all(err <= tol), (key, int(np.argmax(err / np.maximum(tol, 1e-300))))
    assert bool((got[4] > 0).all())
    stats = got[5].cpu().numpy()
    # the sums: the entries' own tolerances, plus the rounding of a tree sum (6 shuffle levels + 2 for the four wavefronts, twice,
    # + ceil(blocks / 256) sequential terms) over sum |term|
    depth = 16 + (rows + 255) // 256
    for k, key in STAT_SUMS:
        terms = GOLD["pw_%s_%s" % (lik, key)][idx]
        tol = float(np.sum(entry_tol(lik, key, idx)) + depth * U * np.sum(np.abs(terms)))
        want = float(np.sum(terms.astype(np.longdouble)))
        print("%s rows %d stats[%d] = sum %s: err %.3e tol %.3e" % (lik, rows, k, key, abs(stats[k] - want), tol))
        assert abs(stats[k] - want) <= tol
    # the maxima: a maximum moves by at most the largest move of an entry
    maxima = list(STAT_MAXIMA) + ([(4, "tau"), (5, "nu")] if moments_only else [(4, "tau_new"), (5, "nu_new")])
    for k, key in maxima:
        terms = np.abs(GOLD["pw_%s_%s" % (lik, key)][idx])
        tol = 0.0 if key in ("tau", "nu") else float(np.max(entry_tol(lik, key, idx)))
        print("%s rows %d stats[%d] = max |%s|: err %.3e tol %.3e" % (lik, rows, k, key, abs(stats[k] - terms.max()), tol))
        assert abs(stats[k] - terms.max()) <= tol
    # the same call twice gives the same bits; NULL moment outputs leave the rest bit-identical
    again = run()
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got, again))
    bare = _ops.ep_sites(LIK_KIND[lik], y, m, mu, sigma2, tau, nu, META["damping"], *rule, moments_only=moments_only, want_moments=False)
    assert bare[2] is None and bare[3] is None and bare[4] is None and torch.equal(bare[5], got[5])
    assert moments_only or (torch.equal(bare[0], got[0]) and torch.equal(bare[1], got[1]))


def test_ep_sites_refuses_other_likelihoods(device):
    v = torch.ones(4, dtype=torch.float64, device=device)
    for kind in (_native.LIK_POISSON, _native.LIK_STUDENT_T):
        with pytest.raises(_native.NativeError, match="-102"):
            _ops.ep_sites(kind, v, None, v, v, v, v, 0.8)
    with pytest.raises(_native.NativeError, match="-10"):
        _ops.ep_sites(_native.LIK_PROBIT, v, None, v, v, 0.0 * v, v, 0.0)
    with pytest.raises(_native.NativeError, match="-11"):
        _ops.ep_sites(_native.LIK_LOGIT, v, None, v, v, 0.0 * v, v, 0.8)


# ---- the golden model cases ---------------------------------------------------------------------------------------------------------
def cuda_model(case):
    inp = lo.case_inputs(case)
    m = eo.build_model(case, inp)
    m.cuda()
    return inp, m


def arr(case, key):
    return GOLD["%s__%s" % (case["name"], key)]


@pytest.mark.parametrize("name", list(CASES))
def test_model_case(device, name):
    case = CASES[name]
    e = case["e64"]
    inp, m = cuda_model(case)
    loss = m.loss()
    loss.backward()
    err = xr.rel_err(loss.item(), case["loss"])
    print("%s: loss %.12f golden %.12f rel err %.2e (tol %.1e), %s, oracle sweeps %d" % (name, loss.item(), case["loss"], err, xr.tol(e["loss"], "loss"),
                                                                                      m.ep_stats, case["sweeps"]))
    assert err <= xr.tol(e["loss"], "loss")
    assert not m.ep_stats["stalled"] and m.ep_stats["sweeps"] < m.max_sweeps
    assert abs(m.ep_stats["sweeps"] - case["sweeps"]) <= 1            # (a change that sits at the threshold may fall either side of it)
    grads = [("variance", m.kernel.variance), ("length_scales", m.kernel.length_scales)]
    if case["mean"] is not None:
        grads.append(("mean", m.mean_function.val))
    for gname, p in grads:
        want = arr(case, "grad_" + gname)
        gerr = xr.rel_err(p.grad.cpu().numpy().reshape(want.shape), want)
        print("   d/d%-14s rel err %.2e of max %.2e (tol %.1e)" % (gname, gerr, np.max(np.abs(want)), xr.tol(e["grad"], "grad")))
        assert gerr <= xr.tol(e["grad"], "grad"), gname
    xs = inp["xs"]
    mean, var = m.predict_f(xs)
    assert mean.shape == (40, 1) and var.shape == (40, 1)
    em, ev = xr.abs_err(mean[:, 0], arr(case, "mean")), xr.abs_err(var[:, 0], arr(case, "var"))
    print("   predict_f: mean %.2e (tol %.1e) var %.2e (tol %.1e)" % (em, xr.tol(e["mean"], "mean"), ev, xr.tol(e["var"], "var")))
    assert em <= xr.tol(e["mean"], "mean") and ev <= xr.tol(e["var"], "var")
    mean2, cov = m.predict_f(xs, diag=False)
    assert xr.abs_err(mean2[:, 0], arr(case, "mean")) <= xr.tol(e["mean"], "mean")
    assert xr.abs_err(np.diag(cov), arr(case, "var")) <= xr.tol(e["var"], "var")
    # predict_y: the likelihood's own map of the golden marginals (stored by the maker).  Its derivatives w.r.t. (mean_f, var_f)
    # are bounded by 0.4 and 0.25 for a Bernoulli likelihood, so the marginals' tolerances propagate with a factor below 1 (4 is
    # kept, as for LaplaceGP), plus 64 ulp for the special functions of two libraries
    py_m, py_v = m.predict_y(xs)
    tol = 4.0 * (xr.tol(e["mean"], "mean") + xr.tol(e["var"], "var")) + 64 * U
    for got, want in ((py_m, arr(case, "py_mean")), (py_v, arr(case, "py_var"))):
        print("   predict_y: err %.2e tol %.1e" % (xr.abs_err(got[:, 0], want), tol))
        assert xr.abs_err(got[:, 0], want) <= tol
    with pytest.raises(NotImplementedError):
        m.predict_y(xs, diag=False)
    with pytest.raises(NotImplementedError):
        m.predict_y_samples(xs, n_samples=2)
    assert m.predict_f_samples(xs, n_samples=3).shape == (3, 40, 1)


@pytest.mark.parametrize("name", list(CASES))
def test_moments_match_at_the_fixed_point(device, name):
    """independent of the goldens: at the converged sites the tilted moments the device computes are the posterior marginals, 1e-7
    relative on every point."""
    _, m = cuda_model(CASES[name])
    with torch.no_grad():
        m.loss()
        st = m._mode_for_predict(m.X)[0]
    em = float(((st.mu_hat - st.mu).abs() / st.mu.abs()).max())
    ev = float(((st.s2_hat - st.sigma2).abs() / st.sigma2).max())
    print("%s: moment matching mean %.2e variance %.2e (min |mu| %.2e)" % (name, em, ev, float(st.mu.abs().min())))
    assert em <= 1e-7 and ev <= 1e-7
    assert bool((st.s2_hat > 0).all()) and bool((st.tau >= 0).all())


def test_warm_and_cold_start_agree(device):
    case = CASES["probit_matern52_ard_513x3"]
    _, m = cuda_model(case)
    with torch.no_grad():
        cold = m.loss()
        cold_stats = dict(m.ep_stats)
        warm = m.loss()
        warm_stats = dict(m.ep_stats)
        m.reset_sites()
        again = m.loss()
        again_stats = dict(m.ep_stats)
        m.warm_start = False
        off = m.loss()
    print("cold %.14f %s warm %.14f %s" % (cold.item(), cold_stats, warm.item(), warm_stats))
    assert xr.rel_err(warm.item(), cold.item()) <= xr.tol(case["e64"]["loss"], "loss")
    assert warm_stats["sweeps"] <= 2 < cold_stats["sweeps"]
    assert torch.equal(again, cold) and again_stats == cold_stats
    assert torch.equal(off, cold) and m.ep_stats == cold_stats


def test_cold_evaluations_repeat_bit_for_bit(device):
    _, m = cuda_model(CASES["logit_matern52_300x3"])
    got = []
    for _ in range(2):
        m.reset_sites()
        m.zero_grad()
        loss = m.loss()
        loss.backward()
        got.append([loss.detach().clone()] + [p.grad.clone() for p in m.parameters() if p.grad is not None])
    assert len(got[0]) == 4 and all(torch.equal(a, b) for a, b in zip(*got))


def test_backward_survives_a_later_forward(device):
    """the factor buffer is reused by the next forward: an earlier node rebuilds its factor (the `generation` check)."""
    _, m = cuda_model(CASES["probit_rbf_300x2"])
    first = m.loss()
    first.backward()
    want = [p.grad.clone() for p in m.parameters() if p.grad is not None]
    m.zero_grad()
    m.reset_sites()
    first = m.loss()
    with torch.no_grad():
        m.kernel.variance.data += 0.1
    m.loss()                                                           # refactorises the shared buffer at other parameters
    with torch.no_grad():
        m.kernel.variance.data -= 0.1
    first.backward()
    got = [p.grad for p in m.parameters() if p.grad is not None]
    assert all(xr.rel_err(a, b) <= 64 * U for a, b in zip(got, want))


def test_adam_steps_follow_the_oracle(device):
    """optimize(method="Adam", max_iter=3) lowers the loss along the trajectory of torch's CPU Adam on the dense fp64 oracle
    (the bound of LaplaceGP's trajectory test: 1e-7 relative)."""
    t = META["trajectory"]
    _, m = cuda_model(CASES[t["case"]])
    with quiet():
        losses, _ = m.optimize(method="Adam", max_iter=t["steps"], learning_rate=t["learning_rate"], verbose=False)
    want = np.asarray(t["losses"])
    err = np.max(np.abs(losses - want) / np.maximum(1.0, np.abs(want)))
    print("ep adam trajectory: losses %s max rel err %.2e" % (losses, err))
    assert losses[-1] < losses[0] and all(a > b for a, b in zip(losses, losses[1:]))
    assert err < 1e-7


def test_multi_start_optimize_is_each_models_own_optimize(device):
    """EPGP restarts take the sequential path of multi_start_optimize: per model, the bits of its own optimize()."""
    case = CASES["probit_rbf_300x2"]
    inp = lo.case_inputs(case)

    def restarts():
        ms = [eo.build_model(dict(case, variance=v, length_scales=[ell]), inp) for v, ell in ((0.3, 1.0), (1.7, 1.0), (8.0, 0.5))]
        for mdl in ms:
            mdl.cuda()
        return ms

    lock, alone = restarts(), restarts()
    assert _lockstep._laplace_groups(lock) == []
    with quiet():
        losses, _ = multi_start_optimize(lock, method="Adam", max_iter=3)
        own = [np.asarray(mdl.optimize(method="Adam", max_iter=3)[0], dtype=np.float64).reshape(-1) for mdl in alone]
    for b in range(3):
        assert np.array_equal(losses[b], own[b]), (losses[b], own[b])
        for p, q in zip(alone[b].parameters(), lock[b].parameters()):
            assert torch.equal(p.data, q.data)
