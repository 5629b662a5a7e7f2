"""The leave-one-out objective of GPR on the GPU: the entry points of csrc/loo.hip at their tile and width edges, every golden case
of tests/golden/make_loo_golden.py through model.cuda(), the dense route, fitting, and the guards that keep the feature out of
everything that existed before it.

Tolerances.  Model quantities: tests/_xref.tol = max(16 e64, FLOOR[what]) with e64 the distance of the oracle's plain-fp64
statement from its long-double one (stored by the maker, or measured here between the two host statements; never against the code
under test); loss and gradients relative to max(1, |reference|) (xr.rel_err), predictions absolute.  gpn_loo_terms: per entry
max(16 e64, 64 * 2^-53 |golden|).  gpn_loo_scale: one rounding, i.e. the bits of the fp64 product.  gpn_loo_grad: FLOOR["dense_grad"]
with e64 of an fp64 numpy evaluation of the same sums."""
import contextlib
import io
import json

import numpy as np
import pytest
import torch

from gptorch_amd import _native, _ops, kernels, likelihoods, mean_functions, rng
from gptorch_amd.models import GPR, batched_loss_and_grad, multi_start_optimize
from tests import _loo_oracle as lo
from tests import _xref as xr
from tests._util import load_npz
from tests.golden import make_loo_golden as maker

pytestmark = pytest.mark.gpu

GOLD = load_npz("loo_cases.npz")
CASES = {c["name"]: c for c in json.loads(str(GOLD["meta"]))["cases"]}
U = 2.0 ** -53
LD = lo.LD
EDGE_N = [1, 63, 64, 65, 128, 129, 257]
EDGE_D = [1, 8, 16, 17]                       # 17 crosses the 16-coordinate staging pass
EDGE_DY = [1, 2, 5]                           # 5 crosses the 4-at-a-time staging of a^T / w^T
GRAD_KINDS = ["Rbf", "Matern52", "Matern32", "Exp", "SqDist", "Periodic"]


def edge_grid():
    """every n with every d (dy dealt round), and every n with every dy (d dealt round): each value of each axis meets every value
    of one other axis."""
    grid = [(n, d, EDGE_DY[(i + j) % 3]) for i, n in enumerate(EDGE_N) for j, d in enumerate(EDGE_D)]
    have = {(n, dy) for n, _, dy in grid}
    grid += [(n, EDGE_D[(i + k) % 4], dy) for i, n in enumerate(EDGE_N) for k, dy in enumerate(EDGE_DY) if (n, dy) not in have]
    return grid


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def cuda(a):
    return torch.tensor(np.asarray(a, dtype=np.float64)).cuda()


def spd(n, seed):
    """a random SPD matrix standing in for P or Q, diagonally dominant enough to be well scaled."""
    g = rng.normal(seed, (n, n + 3))
    return g @ g.T / (n + 3) + 0.5 * np.eye(n)


def lower_buffer(M, ld, device):
    """the lower triangle of M in a [round_up(n, 64), ld] buffer, NaN everywhere else: nothing else may be read."""
    n = M.shape[0]
    buf = torch.full((_ops.round_up(n, 64), ld), float("nan"), dtype=torch.float64, device=device)
    buf[:n, :n] = cuda(np.tril(M) + np.triu(np.full((n, n), np.nan), 1))
    return buf


# ---- the entry points at their edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,dy", edge_grid())
def test_loo_terms(device, n, d, dy):
    p = 0.2 + 3.0 * rng.uniform(100 + n + dy, n)
    a = rng.normal(200 + n + dy, (n, dy))
    ld = int(_native.lib().gpn_factor_ld(n, dy))
    Kinv = torch.full((_ops.round_up(n, 64), ld), float("nan"), dtype=torch.float64, device=device)      # only the diagonal is read
    Kinv.diagonal()[:n] = cuda(p)
    at = cuda(a.T)
    q_ld, v_ld, d_ld, val_ld, t_ld = lo.loo_terms(p, a, LD)
    q_64, v_64, d_64, _, t_64 = lo.loo_terms(p, a, np.float64)
    qt, var, rootd, value = _ops.loo_terms(Kinv, at, n, dy)
    for name, got, gold, plain in (("q", qt.t(), q_ld, q_64), ("var", var, v_ld, v_64), ("rootd", rootd, np.sqrt(d_ld), np.sqrt(d_64))):
        err = np.abs(got.cpu().numpy().astype(LD) - gold)
        tol = np.maximum(16.0 * np.abs(plain.astype(LD) - gold), 64.0 * U * np.abs(gold))
        print("terms n %d dy %d %s: worst err / tol %.3f" % (n, dy, name, float(np.max(err / tol))))
        assert np.all(err <= tol), name
    # value: the entries' own tolerances, plus the rounding of a tree sum (6 shuffle levels + 2 for the four wavefronts +
    # ceil(blocks / 256) sequential terms + 8 levels in the second launch: the allowance of tests/test_gpu_laplace.py) and two more
    # roundings for the constant -1/2 n dy log 2 pi (its own, and its addition), over sum |term| + |constant|
    const = 0.5 * n * dy * np.log(2 * np.pi)
    depth = 16 + (n + 255) // 256 + 2
    tol = float(np.sum(np.maximum(16.0 * np.abs(t_64.astype(LD) - t_ld), 64.0 * U * np.abs(t_ld))) + depth * U * (np.sum(np.abs(t_ld)) + const))
    print("terms n %d dy %d value: err %.3e tol %.3e" % (n, dy, abs(float(value.item() - val_ld)), tol))
    assert abs(float(value.item() - val_ld)) <= tol
    # the same call twice gives the same bits; NULL outputs leave the rest bit-identical
    again = _ops.loo_terms(Kinv, at, n, dy)
    assert all(torch.equal(x, y) for x, y in zip((qt, var, rootd, value), again))
    for keep in range(4):
        flags = [k == keep for k in range(4)]
        only = _ops.loo_terms(Kinv, at, n, dy, None, *flags)
        assert [o is None for o in only] == [not k for k in flags]
        assert torch.equal(only[keep], (qt, var, rootd, value)[keep])


@pytest.mark.parametrize("bad", [0.0, -1.0, float("inf"), float("nan")])
def test_loo_terms_never_clamps_a_bad_precision(device, bad):
    """a p_i that is not a positive finite number: that point's outputs and the value are NaN, every other point keeps its bits."""
    n, dy = 300, 2
    p = 0.2 + 3.0 * rng.uniform(7, n)
    Kinv = torch.zeros(n, n, dtype=torch.float64, device=device)
    Kinv.diagonal().copy_(cuda(p))
    at = cuda(rng.normal(8, (dy, n)))
    good = _ops.loo_terms(Kinv, at, n, dy)
    Kinv[70, 70] = bad
    qt, var, rootd, value = _ops.loo_terms(Kinv, at, n, dy)
    assert bool(torch.isnan(value)) and bool(torch.isnan(var[70])) and bool(torch.isnan(rootd[70])) and bool(torch.isnan(qt[:, 70]).all())
    keep = torch.arange(n, device=device) != 70
    assert torch.equal(qt[:, keep], good[0][:, keep]) and torch.equal(var[keep], good[1][keep]) and torch.equal(rootd[keep], good[2][keep])


@pytest.mark.parametrize("odd_ld", [False, True], ids=["factor_ld", "odd_ld"])
@pytest.mark.parametrize("n", EDGE_N)
def test_loo_scale(device, n, odd_ld):
    """S_ij = P_ij sqrt(d_j) on BOTH triangles from the lower triangle alone, to one rounding (the bits of the fp64 product); a
    sentinel fill shows that nothing outside [n, n] is written.  odd_ld: a leading dimension that rules the 16-byte loads out."""
    lib = _native.lib()
    ld, rows = int(lib.gpn_factor_ld(n, 0)) + (1 if odd_ld else 0), int(lib.gpn_factor_rows(n, 0))
    P = spd(n, 300 + n)
    rootd = 0.1 + rng.uniform(400 + n, n)
    Kinv = lower_buffer(P, ld, device)
    sentinel = -7.25
    S = torch.full((rows, ld), sentinel, dtype=torch.float64, device=device)
    _ops.loo_scale(Kinv, cuda(rootd), n, S)
    low = np.tril(P)
    want = (low + np.tril(P, -1).T) * rootd[None, :]
    assert np.array_equal(S[:n, :n].cpu().numpy(), want)
    assert bool((S[:n, n:] == sentinel).all()) and bool((S[n:] == sentinel).all())
    T = torch.zeros(rows, ld, dtype=torch.float64, device=device)
    _ops.loo_scale(Kinv, cuda(rootd), n, T)
    assert torch.equal(T[:n, :n], S[:n, :n]) and bool((T[:n, n:] == 0).all()) and bool((T[n:] == 0).all())


def host_param_grads(kind, x, var, full_ls, G, ard):
    """sum G dK/d(variance, length_scales) w.r.t. the CONSTRAINED values and tr G, in long double."""
    if kind == "SqDist":                      # K = r^2 (no variance): dK/dell_c = -2 ((x_c - x'_c) / ell_c)^2 / ell_c
        g = np.array([np.sum(ld_(G) * -2 * xr.scaled_sqdist(x[:, c:c + 1], None, full_ls[c:c + 1])) for c in range(x.shape[1])], dtype=LD)
        gv, gl = np.zeros(1, dtype=LD), (g if ard else np.array([g.sum()]))
    else:
        gv, gl = xr.kernel_param_grads(kind, x, None, var, full_ls, G, ard)
        gv = gv / LD(var)
    ls = full_ls if ard else full_ls[:1]
    return np.concatenate([gv, gl / np.asarray(ls, dtype=LD), [np.trace(ld_(G))]])


def ld_(a):
    return np.asarray(a, dtype=LD)


@pytest.mark.parametrize("n,d,dy", edge_grid())
def test_loo_grad(device, n, d, dy):
    """the sweep on a random SPD stand-in for Q and random a, w, against a long-double evaluation of the same sums."""
    i = EDGE_N.index(n) + EDGE_D.index(d) + EDGE_DY.index(dy)
    kind, ard = GRAD_KINDS[i % 6], n % 2 == 1
    x = rng.normal(1000 + 31 * n + d, (n, d)) * (1.0 / np.sqrt(d))
    ls = 0.7 + 0.6 * rng.uniform(2000 + n + d, d if ard else 1)
    full_ls = np.asarray(ls if ard else np.full(d, ls[0]))
    var = 1.3
    Q = spd(n, 500 + n + d)
    a, w = rng.normal(600 + n + dy, (n, dy)), rng.normal(700 + n + dy, (n, dy))

    def G(dt):
        ad, wd = a.astype(dt), w.astype(dt)
        return -Q.astype(dt) + dt(0.5) * (ad @ wd.T + wd @ ad.T)

    want = host_param_grads(kind, x, var, full_ls, G(LD), ard)
    e64 = xr.rel_err(host_param_grads(kind, x, var, full_ls, G(np.float64), ard), want)     # (long-double sums of the fp64 G: a lower bound)
    ldq = int(_native.lib().gpn_factor_ld(n, dy))
    args = (kind, cuda(x), cuda([var]), cuda(ls), lower_buffer(Q, ldq, device), cuda(a.T), cuda(w.T))
    got = _ops.loo_grad(*args)
    err = xr.rel_err(got, want)
    print("grad n %d d %d dy %d %s ard %d: rel err %.2e (e64 %.1e, tol %.1e)" % (n, d, dy, kind, ard, err, e64, xr.tol(e64, "dense_grad")))
    assert got.shape == (2 + ls.size,)
    assert err <= xr.tol(e64, "dense_grad")
    assert torch.equal(got, _ops.loo_grad(*args))


# ---- the golden model cases ---------------------------------------------------------------------------------------------------------
def build_model(case, objective="loo", inputs=None):
    x, y = maker.case_inputs(case) if inputs is None else inputs
    ls = np.asarray(case["length_scales"], dtype=np.float64) if case["ARD"] else float(case["length_scales"][0])
    k = getattr(kernels, case["kind"])(case["d"], variance=float(case["variance"]), length_scales=ls, ARD=bool(case["ARD"]))
    mean = None if case["mean"] is None else mean_functions.Constant(case["dy"], torch.tensor(case["mean"], dtype=torch.float64))
    m = GPR(x, y, k, mean_function=mean, likelihood=likelihoods.Gaussian(variance=float(case["noise"])), objective=objective)
    m.cuda()
    return m


def arr(case, key):
    return GOLD["%s__%s" % (case["name"], key)]


_REFS = {}


def oracle(name):
    """the two host statements of a golden case, built once for every test that needs more than the stored numbers"""
    if name not in _REFS:
        _REFS[name] = maker.build(CASES[name])
    return _REFS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_model_case(device, name):
    case = CASES[name]
    e = case["e64"]
    m = build_model(case)
    loss = m.loss()
    loss.backward()
    err = xr.rel_err(loss.item(), case["loss"])
    print("%s: loss %.12f golden %.12f rel err %.2e (tol %.1e)" % (name, loss.item(), case["loss"], err, xr.tol(e["loss"], "loss")))
    assert loss.shape == (1,) and err <= xr.tol(e["loss"], "loss")
    grads = [("variance", m.kernel.variance), ("length_scales", m.kernel.length_scales), ("noise", m.likelihood.variance)]
    if case["mean"] is not None:
        grads.append(("mean", m.mean_function.val))
    for gname, p in grads:
        want = arr(case, "grad_" + gname)
        gerr = xr.rel_err(p.grad.cpu().numpy().reshape(want.shape), want)
        print("   d/d%-14s rel err %.2e of max %.2e (tol %.1e)" % (gname, gerr, np.max(np.abs(want)), xr.tol(e["grad"], "grad")))
        assert gerr <= xr.tol(e["grad"], "grad"), gname
    mean, var = m.loo_predict()
    assert mean.shape == (case["n"], case["dy"]) and var.shape == (case["n"], case["dy"]) and not mean.requires_grad
    em, ev = xr.abs_err(mean, arr(case, "mean")), xr.abs_err(var, arr(case, "var"))
    print("   loo_predict: mean %.2e (tol %.1e) var %.2e (tol %.1e)" % (em, xr.tol(e["mean"], "mean"), ev, xr.tol(e["var"], "var")))
    assert em <= xr.tol(e["mean"], "mean") and ev <= xr.tol(e["var"], "var")
    if case["refits"]:
        # ... and against models that really never saw the point
        rm, rv = xr.abs_err(mean, arr(case, "refit_mean")), xr.abs_err(var[:, 0], arr(case, "refit_var"))
        print("   loo_predict vs %d refits: mean %.2e var %.2e" % (case["n"], rm, rv))
        assert rm <= xr.tol(e["mean"], "mean") and rv <= xr.tol(e["var"], "var")
    # no priors: the objective is the loss's negative, bit for bit, and log_likelihood() is still the LML
    assert torch.equal(m.loo_log_predictive(), -loss.detach())
    lml = build_model(case, objective="lml")
    assert torch.equal(m.log_likelihood(), lml.log_likelihood()) and not torch.equal(m.log_likelihood(), m.loo_log_predictive())


# ---- the dense route ------------------------------------------------------------------------------------------------------------------
def test_dense_node_on_a_native_kernel_matrix(device):
    """DenseLooLik.apply on the native K of the Matern52 case: value, the returned G entrywise, -w and tr G against the oracle."""
    name = "matern52_ard_257x3"
    case, (ref, _) = CASES[name], oracle(name)
    e = case["e64"]
    x, y = maker.case_inputs(case)
    X = cuda(x)
    K = _ops.kernel_matrix(case["kind"], X, None, cuda([case["variance"]]), cuda(case["length_scales"])).requires_grad_(True)
    R = (cuda(y) - cuda(case["mean"])[None, :]).requires_grad_(True)
    noise = cuda([case["noise"]]).requires_grad_(True)
    value = _ops.DenseLooLik.apply(K, R, noise)
    value.backward()
    G, w = ref.G()
    err = xr.rel_err(value.item(), -case["loss"])
    eg, ew = xr.abs_err(K.grad, G), xr.abs_err(R.grad, -w)
    et = xr.rel_err(noise.grad.item(), float(np.trace(G)))
    print("dense node: value %.2e (tol %.1e) G %.2e of max %.2e, -w %.2e (tol %.1e) tr G %.2e (tol %.1e)"
          % (err, xr.tol(e["loss"], "loss"), eg, float(np.max(np.abs(G))), ew, xr.tol(e["dense_grad"], "dense_grad"), et, xr.tol(e["grad"], "grad")))
    assert value.shape == (1,) and err <= xr.tol(e["loss"], "loss")
    assert eg <= xr.tol(e["dense_grad"], "dense_grad") and ew <= xr.tol(e["dense_grad"], "dense_grad")
    assert et <= xr.tol(e["grad"], "grad")


def test_sum_of_two_rbf_is_one_rbf(device):
    """GPR(Rbf(v1) + Rbf(v2), objective="loo") with one length scale is the model Rbf(v1 + v2): value and gradients against the
    oracle at v = v1 + v2, the raw-variance and raw-length-scale gradients split as v1 / v and v2 / v."""
    n, d, v1, v2, ell, noise = 150, 2, 0.9, 0.5, 0.8, 0.05
    x, y = rng.make_regression(n, d, 1, seed=241)
    ref, t64 = lo.make_pair(x, y, "Rbf", v1 + v2, ell, noise)
    loss64, g64 = t64.loss_grads_with_mean()
    want = ref.loss_grads()
    e_loss, e_grad = xr.rel_err(loss64, ref.loss()), max(xr.rel_err(a, b) for a, b in zip(g64, want))
    k1, k2 = kernels.Rbf(d, variance=v1, length_scales=ell), kernels.Rbf(d, variance=v2, length_scales=ell)
    m = GPR(x, y, k1 + k2, likelihood=likelihoods.Gaussian(variance=noise), objective="loo")
    m.cuda()
    loss = m.loss()
    loss.backward()
    print("sum kernel: loss rel err %.2e (tol %.1e)" % (xr.rel_err(loss.item(), ref.loss()), xr.tol(e_loss, "loss")))
    assert xr.rel_err(loss.item(), ref.loss()) <= xr.tol(e_loss, "loss")
    v = LD(v1) + LD(v2)
    for k, share in ((k1, LD(v1) / v), (k2, LD(v2) / v)):
        for p, g in ((k.variance, want[0]), (k.length_scales, want[1])):
            gerr = xr.rel_err(p.grad.cpu().numpy().reshape(-1), share * g)
            print("   rel err %.2e (tol %.1e)" % (gerr, xr.tol(e_grad, "grad")))
            assert gerr <= xr.tol(e_grad, "grad")
    assert xr.rel_err(m.likelihood.variance.grad.cpu().numpy(), want[2]) <= xr.tol(e_grad, "grad")
    mean, var = m.loo_predict()
    wm, wv = ref.loo_predict()
    assert xr.abs_err(mean, wm) <= xr.tol(xr.abs_err(t64.loo_predict()[0], wm), "mean")
    assert xr.abs_err(var, wv) <= xr.tol(xr.abs_err(t64.loo_predict()[1], wv), "var")


# ---- fitting ----------------------------------------------------------------------------------------------------------------------------
def test_adam_follows_the_fp64_statement(device):
    case = CASES["rbf_300x2"]
    m = build_model(case)
    with quiet():
        losses, _ = m.optimize(method="Adam", max_iter=3, learning_rate=0.05, verbose=False)
    _, t64 = maker.build(case)
    want = t64.optimize_adam(max_iter=3, learning_rate=0.05)
    for got, w in zip(losses, want):
        print("adam: %.12f vs %.12f" % (got, w))
        assert xr.rel_err(got, w) <= xr.FLOOR["loss"]


def test_scipy_lbfgsb_lowers_the_loss(device):
    m = build_model(CASES["rbf_300x2"])
    first = m.loss().item()
    with quiet():
        res = m.optimize(method="L-BFGS-B", max_iter=5, verbose=False)
    assert np.isfinite(res.fun) and res.fun < first


def test_a_noise_prior_enters_the_loss_once(device):
    m = build_model(CASES["rbf_300x2"])
    plain = m.loss().detach()
    prior = torch.distributions.Gamma(torch.tensor(2.0, dtype=torch.float64, device=device), torch.tensor(10.0, dtype=torch.float64, device=device))
    m.likelihood.variance.prior = prior
    with_prior = m.loss()
    lp = prior.log_prob(m.likelihood.variance.transform()).sum().detach()
    assert lp.item() != 0.0 and torch.equal(with_prior.detach(), -(-plain + lp))
    with_prior.backward()
    assert m.likelihood.variance.grad is not None and bool(torch.isfinite(m.likelihood.variance.grad).all())


# ---- no leak into what exists ---------------------------------------------------------------------------------------------------------
def restarts(case, objectives, inputs):
    """models of one case from different starting points (the k-th: variance * (1 + k / 4), noise * (1 + k / 2))"""
    out = []
    for k, obj in enumerate(objectives):
        c = dict(case, variance=case["variance"] * (1 + k / 4), noise=case["noise"] * (1 + k / 2))
        out.append(build_model(c, objective=obj, inputs=inputs))
    return out


def state(m):
    return [p.detach().clone() for p in m.parameters()]


def test_multi_start_keeps_loo_models_out_of_the_lockstep_groups(device):
    """two ordinary restarts and one objective="loo" model in one multi_start_optimize: the ordinary two get, bit for bit, what a
    call without the third gives them; the third gets what its own optimize() gives."""
    case = CASES["rbf_300x2"]
    inputs = tuple(torch.tensor(t) for t in maker.case_inputs(case))
    a, b, c = restarts(case, ["lml", "lml", "loo"], inputs)
    a2, b2, c2 = restarts(case, ["lml", "lml", "loo"], inputs)
    with quiet():
        mixed, _ = multi_start_optimize([a, b, c], method="Adam", max_iter=3, verbose=False, learning_rate=0.05)
        alone, _ = multi_start_optimize([a2, b2], method="Adam", max_iter=3, verbose=False, learning_rate=0.05)
        own, _ = c2.optimize(method="Adam", max_iter=3, verbose=False, learning_rate=0.05)
    assert np.array_equal(mixed[:2], alone) and np.array_equal(mixed[2], own)
    for got, want in ((a, a2), (b, b2), (c, c2)):
        assert all(torch.equal(p, q) for p, q in zip(state(got), state(want)))
    assert not np.array_equal(mixed[2], mixed[1])


def test_batched_loss_and_grad_evaluates_a_loo_model_by_itself(device):
    case = CASES["rbf_300x2"]
    inputs = tuple(torch.tensor(t) for t in maker.case_inputs(case))
    ms = restarts(case, ["lml", "loo", "lml"], inputs)
    single = restarts(case, ["lml", "loo", "lml"], inputs)
    out = batched_loss_and_grad(ms)
    for m, s, o in zip(ms, single, out):
        loss = s.loss()
        loss.backward()
        assert torch.equal(o, loss.detach())
        assert all(torch.equal(p.grad, q.grad) for p, q in zip(m.parameters(), s.parameters()) if q.grad is not None)


def test_capture_falls_back_to_the_ordinary_loop(device):
    case = CASES["rbf_300x2"]
    m, m2 = build_model(case), build_model(case)
    assert not m._can_capture("Adam") and build_model(case, objective="lml")._can_capture("Adam")
    with quiet():
        captured, _ = m.optimize(method="Adam", max_iter=3, verbose=False, capture=True)
        ordinary, _ = m2.optimize(method="Adam", max_iter=3, verbose=False)
    assert np.array_equal(captured, ordinary)


def test_default_objective_is_the_untouched_lml_path(device):
    """a default GPR: loss() and its gradients carry the bits of GPRLogLik.apply called directly on the same inputs."""
    case = CASES["matern52_ard_257x3"]
    m, twin = build_model(case, objective="lml"), build_model(case, objective="lml")
    assert m.objective == "lml"
    loss = m.loss()
    loss.backward()
    k = twin.kernel
    direct = -(_ops.GPRLogLik.apply(twin.X, twin.Y - twin.mean_function(twin.X), k.variance.transform(), k.length_scales.transform(),
                                    twin.likelihood.variance.transform(), k._kind, {}) + 0.0)
    direct.backward()
    assert torch.equal(loss.detach(), direct.detach())
    for p, q in zip(m.parameters(), twin.parameters()):
        assert torch.equal(p.grad, q.grad)
