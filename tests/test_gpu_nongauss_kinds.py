"""The tile kernels that LaplaceGP and EPGP stand on -- gpn_laplace_system, _matvec, _diag, _grad: kmat_kernel<KIND, true>,
lap_rows_kernel<KIND, 0 | 1>, lap_grad_kernel<KIND> -- for ALL five covariance kinds, on the planted points of
tests/_refine_ref.points (repeated rows, pairs under and just above the clamp, a row 1000 ell away, Periodic's sign changes).

The checks are the existing forms of tests/test_gpu_laplace.py, per kind: the long-double sums at xr.tol(e64, "dense_grad") with
e64 from the fp64 statement of the same sums (tests/_laplace_oracle.kern, which now knows Exp and Periodic), B within
4 * 2^-53 |B_ij| of the scaled gpn_kernel_matrix entries, NaN above Binv's diagonal, sentinel padding, the same call twice the
same bits; the lock-step forms bit-identical per slot to the single calls; and a weight pattern that lives only on pairs under
the clamp, whose length-scale gradient is exactly 0 for every kind but Rbf.

Model level (cases and oracles: tests/_nongauss_cases.py): LaplaceGP and EPGP through model.cuda() with Matern32, Exp and Periodic
(d = 1, planted points) against the dense host oracles in long double, at the tolerances of the test_model_case of
tests/test_gpu_laplace.py and tests/test_gpu_ep.py; two restarts of every case through multi_start_optimize, each model's values
those of its own run bit for bit; and LaplaceGP over a Periodic kernel at d = 2 (an indefinite K), which must raise from the
factorisation's info.  tests/test_kind_ref_host.py shows on the host that every case's inputs separate the five kinds by a million
tolerances."""
import numpy as np
import pytest
import torch

from gptorch_amd import _native, _ops, kernels, likelihoods, rng
from gptorch_amd.models import LaplaceGP
from tests import _laplace_oracle as lo
from tests import _nongauss_cases as nc
from tests import _refine_ref as rr
from tests import _xref as xr

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = xr.LD
KINDS, CASES = nc.KINDS, nc.TILE_CASES
SENTINEL = -7.25


def cuda(a):
    return torch.tensor(np.asarray(a, dtype=np.float64)).cuda()


@pytest.mark.parametrize("kind,n,d,ard", CASES)
def test_tile_kernels_of_every_kind(device, kind, n, d, ard):
    t = nc.tile_inputs(kind, n, d, ard)
    x, var, ls, full_ls, s = t["x"], t["var"], t["ls"], t["full_ls"], t["s"]
    a, u, d1, vec, Binv = t["a"], t["u"], t["d1"], t["vec"], t["Binv"]
    ref = nc.tile_refs(t, kind)
    X, v, l = cuda(x), cuda([var]), cuda(ls)

    # gpn_laplace_system: B_ij = delta_ij + s_i s_j k_ij with the bits of gpn_kernel_matrix's k_ij -- three roundings
    ld = int(_native.lib().gpn_factor_ld(n, 1))
    A = torch.full((n + 3, ld), SENTINEL, dtype=torch.float64, device=device)
    _ops.laplace_system(kind, X, v, l, cuda(s), A, ld)
    K = _ops.kernel_matrix(kind, X, None, v, l, out=torch.zeros(n, ld, dtype=torch.float64, device=device), ldk=ld, lower=True)[:, :n]
    want = np.outer(s, s).astype(LD) * K.cpu().numpy().astype(LD) + np.eye(n, dtype=LD)     # (s_i s_j rounded once, as the kernel does)
    got = A[:n, :n].cpu().numpy()
    low = np.tril(np.ones((n, n), dtype=bool))
    err = np.abs(got.astype(LD) - want)[low]                     # (the far row's k_ij underflow to 0: B_ij = 0 exactly there)
    print("system %s n %d d %d ard %d: worst err %.2f ulp" % (kind, n, d, ard, float(np.max(err / np.maximum(np.abs(want[low]), LD(1e-300))) / U)))
    assert np.all(err <= 4 * U * np.abs(want[low]))
    assert np.all(got[~low] == SENTINEL)
    assert bool((A[:n, n:] == SENTINEL).all()) and bool((A[n:] == SENTINEL).all())
    again = torch.full((n + 3, ld), SENTINEL, dtype=torch.float64, device=device)
    _ops.laplace_system(kind, X, v, l, cuda(s), again, ld)
    assert torch.equal(A, again)
    # ... and the k_ij themselves are this kind's: the long-double kernel on the same points
    Kld, tolK, _ = ref["K"]
    assert xr.abs_err(K.cpu().numpy()[low], Kld[low]) <= tolK

    # gpn_laplace_matvec / _diag / _grad against long double
    Bl = cuda(np.tril(Binv) + np.triu(np.full((n, n), np.nan), 1))            # the upper triangle must never be read
    calls = {"matvec": lambda: _ops.laplace_matvec(kind, X, v, l, cuda(vec)),
             "diag": lambda: _ops.laplace_diag(kind, X, v, l, cuda(s), Bl),
             "grad": lambda: _ops.laplace_grad(kind, X, v, l, cuda(s), Bl, cuda(a), cuda(u), cuda(d1))}
    for name in ("matvec", "diag", "grad"):
        want_v, tol, _ = ref[name]
        got_v = calls[name]()
        err = xr.rel_err(got_v, want_v)
        print("%s %s n %d d %d ard %d: rel err %.2e (tol %.1e, err / tol %.3f)" % (name, kind, n, d, ard, err, tol, err / tol))
        assert err <= tol, name
        assert torch.equal(got_v, calls[name]())


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_weights_under_the_clamp_give_no_length_scale_gradient(device, kind, ard):
    """G nonzero only on off-diagonal pairs with r^2 < 1e-40 (a = u = d1 = 0, Binv supported there): every kind but Rbf has
    dK/dell = 0 under the clamp, exactly -- Exp's K e^-r / r and Periodic's sin r / r must not be evaluated at the clamped r."""
    n, d = 65, 2
    x, var, ls, full_ls, seed = nc.problem(kind, n, d, ard)
    r2 = np.asarray(xr.scaled_sqdist(x, None, full_ls))
    dead = (r2 < xr.CLAMP) & ~np.eye(n, dtype=bool)
    assert dead.sum() >= 4                                       # the planted repeated rows and the pair 1e-21 ell apart
    Binv = np.where(dead, 1.0 + rng.uniform(seed + 5, n * n).reshape(n, n), 0.0)
    Binv = np.tril(Binv) + np.tril(Binv, -1).T
    Bl = cuda(np.tril(Binv) + np.triu(np.full((n, n), np.nan), 1))
    s = 0.5 + rng.uniform(seed + 6, n)
    zero = cuda(np.zeros(n))
    got = _ops.laplace_grad(kind, cuda(x), cuda([var]), cuda(ls), cuda(s), Bl, zero, zero, zero).cpu().numpy()
    # the variance output is the plain sum: -1/2 sum s_i s_j Binv_ij k_ij / variance with k_ij = variance (r = 0 to 1e-20)
    want_var = -0.5 * np.sum(np.outer(s, s) * Binv)
    assert abs(got[0] - want_var) <= 64 * U * abs(want_var)
    if kind == "Rbf":                                            # no clamp: dK/dell = K r^2 / ell, r^2 <= 1e-40 here
        assert np.all(np.abs(got[1:]) <= 1e-38 * abs(want_var))
    else:
        assert np.all(got[1:] == 0.0), got


@pytest.mark.parametrize("stacked", [False, True], ids=["shared_x", "stacked_x"])
@pytest.mark.parametrize("kind", KINDS)
def test_lockstep_slots_equal_the_single_calls(device, kind, stacked):
    """B = 3 models with their own hyper-parameters, shared points (sX = 0) and points per model: every slot of every lock-step
    entry carries the bits of its single call."""
    B, n, d = 3, 129, 2
    ard = True
    seed = 900 + 11 * KINDS.index(kind)
    lss = np.stack([rr.length_scales(d, ard, seed + b, 0.9 + 0.1 * b) for b in range(B)])
    xs = [rr.points(seed + 10 + b, n, d, lss[b, 0], first=b) for b in range(B)]
    X = cuda(np.stack(xs)) if stacked else cuda(xs[0])
    Xb = lambda b: X[b] if stacked else X
    var, ls = cuda([0.6, 1.3, 2.1]), cuda(lss)
    vec = lambda k: cuda(rng.normal(seed + 20 + k, (B, n)))
    s = cuda(0.05 + 2.0 * rng.uniform(seed + 40, B * n).reshape(B, n))

    fb = _ops.FactorBatch(B, n, 1, device)
    fb.A.fill_(SENTINEL)
    _ops.laplace_system_batched(kind, X, var, ls, s, fb)
    slots = fb.A.view(B, fb.rows, fb.ld)
    for b in range(B):
        A = torch.full((fb.rows, fb.ld), SENTINEL, dtype=torch.float64, device=device)
        _ops.laplace_system(kind, Xb(b), var[b:b + 1], ls[b], s[b], A, fb.ld)
        assert torch.equal(slots[b], A), b
    v = vec(1)
    got = _ops.laplace_matvec_batched(kind, X, var, ls, v)
    for b in range(B):
        assert torch.equal(got[b], _ops.laplace_matvec(kind, Xb(b), var[b:b + 1], ls[b], v[b])), b
    rp = _ops.round_up(n, 64)
    Binv = torch.zeros(B, rp, fb.ld, dtype=torch.float64, device=device)
    Binv[:, :n, :n] = cuda(np.stack([nc.spd(n, seed + 70 + b) for b in range(B)]))
    got = _ops.laplace_diag_batched(kind, X, var, ls, s, Binv, fb.ld, rp * fb.ld)
    for b in range(B):
        assert torch.equal(got[b], _ops.laplace_diag(kind, Xb(b), var[b:b + 1], ls[b], s[b], Binv[b])), b
    a, u, d1 = vec(2), vec(3), vec(4)
    got = _ops.laplace_grad_batched(kind, X, var, ls, s, Binv, fb.ld, rp * fb.ld, a, u, d1)
    for b in range(B):
        assert torch.equal(got[b], _ops.laplace_grad(kind, Xb(b), var[b:b + 1], ls[b], s[b], Binv[b], a[b], u[b], d1[b])), b


def test_laplacegp_refuses_an_indefinite_periodic_kernel(device):
    """Periodic at d = 2 is not positive semi-definite: on the planted points lambda_min(K) is far below -1 / max W, B = I +
    W^1/2 K W^1/2 is indefinite, and loss() must raise from the factorisation's info -- no NaN, no finite value."""
    n, d = 65, 2
    x = rr.points(31, n, d, 1.0)
    y = (rng.uniform(32, n) < 0.5).astype(np.float64)[:, None]
    K = np.asarray(xr.K("Periodic", x, None, rr.VAR, np.ones(d)), dtype=np.float64)
    lam = np.linalg.eigvalsh(K).min()
    assert lam < -8.0, lam                                       # probit's W at f = 0 is 2 / pi: 1 + W lambda_min < 0
    m = LaplaceGP(x, y, kernels.Periodic(d, variance=rr.VAR, length_scales=1.0), likelihoods.Bernoulli("probit"))
    m.cuda()
    with pytest.raises(_native.NativeError, match="info = "):
        m.loss()


# ---- LaplaceGP through model.cuda() for the kinds no golden case holds -----------------------------------------------------------------
# The oracles run here, on the host, in long double and in fp64 (about a second per case): e64 is their distance, the tolerances
# are those of tests/test_gpu_laplace.py::test_model_case.
@pytest.mark.parametrize("case", nc.MODEL_CASES, ids=[c["name"] for c in nc.MODEL_CASES])
def test_laplacegp_model_case(device, case):
    gold = nc.oracle_numbers(case)
    e, inp = gold["e64"], gold["inp"]
    m = lo.build_model(case, inp)
    m.cuda()
    loss = m.loss()
    loss.backward()
    err = xr.rel_err(loss.item(), gold["loss"])
    print("%s: loss %.12f oracle %.12f rel err %.2e (tol %.1e), %s" % (case["name"], loss.item(), gold["loss"], err, xr.tol(e["loss"], "loss"),
                                                                      m.newton_stats))
    assert err <= xr.tol(e["loss"], "loss")
    for gname, p in (("variance", m.kernel.variance), ("length_scales", m.kernel.length_scales)):
        want = gold["grad_" + gname]
        gerr = xr.rel_err(p.grad.cpu().numpy().reshape(want.shape), want)
        print("   d/d%-14s rel err %.2e of max %.2e (tol %.1e)" % (gname, gerr, np.max(np.abs(want)), xr.tol(e["grad"], "grad")))
        assert gerr <= xr.tol(e["grad"], "grad"), gname
    xs = inp["xs"]
    mean, var = m.predict_f(xs)
    mean2, cov = m.predict_f(xs, diag=False)
    em, ev, ec = xr.abs_err(mean[:, 0], gold["mean"]), xr.abs_err(var[:, 0], gold["var"]), xr.abs_err(cov, gold["cov"])
    print("   predict_f: mean %.2e (tol %.1e) var %.2e (tol %.1e) cov %.2e (tol %.1e)"
          % (em, xr.tol(e["mean"], "mean"), ev, xr.tol(e["var"], "var"), ec, xr.tol(e["cov"], "var")))
    assert em <= xr.tol(e["mean"], "mean") and ev <= xr.tol(e["var"], "var") and ec <= xr.tol(e["cov"], "var")
    assert xr.abs_err(mean2[:, 0], gold["mean"]) <= xr.tol(e["mean"], "mean")
    # predict_y: the likelihood's own map of the oracle's marginals (the bound of tests/test_gpu_laplace.py::test_model_case)
    gm, gvv = torch.tensor(gold["mean"])[:, None], torch.tensor(gold["var"])[:, None]
    wy_m, wy_v = m.likelihood.predict_mean_variance(gm, gvv)
    py_m, py_v = m.predict_y(xs)
    for got, want in ((py_m, wy_m), (py_v, wy_v)):
        scale = max(1.0, float(want.abs().max()))
        tol = (4.0 * (xr.tol(e["mean"], "mean") + xr.tol(e["var"], "var")) + 64 * U) * scale
        assert xr.abs_err(got, want.numpy()) <= tol


# ---- EPGP through model.cuda() for the same kinds ------------------------------------------------------------------------------------------
# tests/golden/make_ep_golden.py's model_case, computed here (about a second per case); the tolerances of
# tests/test_gpu_ep.py::test_model_case.
@pytest.mark.parametrize("case", nc.EP_CASES, ids=[c["name"] for c in nc.EP_CASES])
def test_epgp_model_case(device, case):
    from tests import _ep_oracle as eo
    gold = nc.ep_golden(case)
    e, inp = gold["e64"], gold["inp"]
    m = eo.build_model(case, inp)
    m.cuda()
    loss = m.loss()
    loss.backward()
    err = xr.rel_err(loss.item(), gold["loss"])
    print("%s: loss %.12f oracle %.12f rel err %.2e (tol %.1e), %s, oracle sweeps %d" % (case["name"], loss.item(), gold["loss"], err,
                                                                                        xr.tol(e["loss"], "loss"), m.ep_stats, gold["sweeps"]))
    assert err <= xr.tol(e["loss"], "loss")
    assert not m.ep_stats["stalled"] and m.ep_stats["sweeps"] < m.max_sweeps
    assert abs(m.ep_stats["sweeps"] - gold["sweeps"]) <= 1
    for gname, p in (("variance", m.kernel.variance), ("length_scales", m.kernel.length_scales)):
        want = gold["grad_" + gname]
        gerr = xr.rel_err(p.grad.cpu().numpy().reshape(want.shape), want)
        print("   d/d%-14s rel err %.2e of max %.2e (tol %.1e)" % (gname, gerr, np.max(np.abs(want)), xr.tol(e["grad"], "grad")))
        assert gerr <= xr.tol(e["grad"], "grad"), gname
    xs = inp["xs"]
    mean, var = m.predict_f(xs)
    em, ev = xr.abs_err(mean[:, 0], gold["mean"]), xr.abs_err(var[:, 0], gold["var"])
    print("   predict_f: mean %.2e (tol %.1e) var %.2e (tol %.1e)" % (em, xr.tol(e["mean"], "mean"), ev, xr.tol(e["var"], "var")))
    assert em <= xr.tol(e["mean"], "mean") and ev <= xr.tol(e["var"], "var")
    mean2, cov = m.predict_f(xs, diag=False)
    assert xr.abs_err(mean2[:, 0], gold["mean"]) <= xr.tol(e["mean"], "mean")
    assert xr.abs_err(np.diag(cov), gold["var"]) <= xr.tol(e["var"], "var")
    # predict_y: the likelihood's own map of the oracle's marginals
    lik = likelihoods.Bernoulli(case["lik"])
    lik.num_gauss_hermite_points = int(case["H"])
    wy_m, wy_v = lik.predict_mean_variance(torch.tensor(gold["mean"])[:, None], torch.tensor(gold["var"])[:, None])
    py_m, py_v = m.predict_y(xs)
    tol = 4.0 * (xr.tol(e["mean"], "mean") + xr.tol(e["var"], "var")) + 64 * U
    for got, want in ((py_m, wy_m), (py_v, wy_v)):
        assert xr.abs_err(got[:, 0], want[:, 0].numpy()) <= tol


# ---- two restarts of every model case in lock step: each model's values are those of its own run, bit for bit -----------------------------
@pytest.mark.parametrize("case", nc.MODEL_CASES + nc.EP_CASES, ids=[c["name"] for c in nc.MODEL_CASES + nc.EP_CASES])
def test_two_restarts_in_lock_step_equal_their_own_runs(device, case):
    import contextlib
    import io
    from gptorch_amd.models import multi_start_optimize
    from tests import _ep_oracle as eo
    build = eo.build_model if case in nc.EP_CASES else lo.build_model
    inp = nc.model_inputs(case)

    def restarts():
        out = []
        for fac_v, fac_l in ((1.0, 1.0), (1.4, 0.85)):
            mdl = build(dict(case, variance=case["variance"] * fac_v, length_scales=list(np.asarray(case["length_scales"]) * fac_l)), inp)
            mdl.cuda()
            out.append(mdl)
        return out
    lock, alone = restarts(), restarts()
    with contextlib.redirect_stdout(io.StringIO()):
        losses, _ = multi_start_optimize(lock, method="Adam", max_iter=1)
        own = [np.asarray(mdl.optimize(method="Adam", max_iter=1)[0], dtype=np.float64).reshape(-1) for mdl in alone]
    for b in range(2):
        assert np.array_equal(losses[b], own[b]), (b, losses[b], own[b])
        assert np.all(np.isfinite(own[b]))
        for p, q in zip(alone[b].parameters(), lock[b].parameters()):
            assert torch.equal(p.data, q.data), b
