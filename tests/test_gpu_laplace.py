"""LaplaceGP on the GPU: the entry points of csrc/laplace.hip at their tile and width edges, and every golden model case of
tests/golden/make_laplace_golden.py through model.cuda() and the C ABI.

Tolerances.  Model quantities: tests/_xref.tol = max(16 e64, FLOOR[what]) with e64 the distance of the oracle's plain-fp64
statement from its long-double one (stored by the maker; never measured against the code under test); loss and gradients
relative to max(1, |reference|) (xr.rel_err), predictions absolute.  Pointwise quantities: max(16 e64, 64 * 2^-53 |golden|) per
entry.  The sweeps of gpn_laplace_diag / gpn_laplace_grad: FLOOR["dense_grad"] with e64 of an fp64 numpy evaluation of the same
sums."""
import contextlib
import io
import json

import numpy as np
import pytest
import torch

from gptorch_amd import _native, _ops, kernels, likelihoods, rng
from gptorch_amd.models import LaplaceGP
from tests import _laplace_oracle as lo
from tests import _xref as xr
from tests._util import load_npz

pytestmark = pytest.mark.gpu

GOLD = load_npz("laplace_cases.npz")
META = json.loads(str(GOLD["meta"]))
CASES = {c["name"]: c for c in META["cases"]}
U = 2.0 ** -53
LIK_KIND = {"probit": _native.LIK_PROBIT, "logit": _native.LIK_LOGIT, "poisson": _native.LIK_POISSON}
EDGE_N = [1, 63, 64, 65, 128, 129, 257]
EDGE_D = [1, 8, 16, 17]                       # 17 crosses the 16-coordinate staging pass


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def cuda(a):
    return torch.tensor(np.asarray(a, dtype=np.float64)).cuda()


# ---- gpn_lik_derivs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lik", ["probit", "logit", "poisson"])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257, 513, 1000])
def test_lik_derivs_match_the_goldens(device, lik, rows):
    npts = GOLD["pw_%s_f" % lik].size
    idx = (np.arange(rows) * 7 + rows) % npts                         # the golden points, dealt over the rows
    f, y = cuda(GOLD["pw_%s_f" % lik][idx]), cuda(GOLD["pw_%s_y" % lik][idx])
    value, d1, w, d3 = _ops.lik_derivs(LIK_KIND[lik], f, y)
    for name, got in (("d1", d1), ("W", w), ("d3", d3)):
        gold, e64 = GOLD["pw_%s_%s" % (lik, name)][idx], GOLD["pw_%s_%s_e64" % (lik, name)][idx]
        err, tol = np.abs(got.cpu().numpy() - gold), np.maximum(16.0 * e64, 64.0 * U * np.abs(gold))
        print("%s rows %d %s: worst err / tol %.3f" % (lik, rows, name, np.max(err / np.maximum(tol, 1e-300))))
        assert np.all(err <= tol), (name, int(np.argmax(err / np.maximum(tol, 1e-300))))
    # value = sum lp: the entries' own tolerances, plus the rounding of a tree sum (6 shuffle levels + 2 for the four wavefronts
    # + ceil(blocks / 256) sequential terms + 8 levels in the second launch) over sum |lp|
    lp, e64 = GOLD["pw_%s_lp" % lik][idx], GOLD["pw_%s_lp_e64" % lik][idx]
    depth = 16 + (rows + 255) // 256
    tol = float(np.sum(np.maximum(16.0 * e64, 64.0 * U * np.abs(lp))) + depth * U * np.sum(np.abs(lp)))
    want = float(np.sum(lp.astype(np.longdouble)))
    print("%s rows %d value: err %.3e tol %.3e" % (lik, rows, abs(value.item() - want), tol))
    assert abs(value.item() - want) <= tol
    # NULL outputs leave the rest bit-identical; the same call twice gives the same bits
    again = _ops.lik_derivs(LIK_KIND[lik], f, y)
    assert all(torch.equal(a, b) for a, b in zip((value, d1, w, d3), again))
    for keep in range(4):
        flags = [k == keep for k in range(4)]
        only = _ops.lik_derivs(LIK_KIND[lik], f, y, *flags)
        assert [o is None for o in only] == [not k for k in flags]
        assert torch.equal(only[keep], (value, d1, w, d3)[keep])


def test_lik_derivs_refuses_student_t(device):
    f = torch.zeros(4, dtype=torch.float64, device=device)
    with pytest.raises(_native.NativeError, match="-102"):
        _ops.lik_derivs(_native.LIK_STUDENT_T, f, f)


# ---- the tile entry points at their edges -----------------------------------------------------------------------------------------------
def edge_problem(n, d):
    """points, hyper-parameters and a kind for an (n, d) edge: ARD for odd n, Matern52 / Rbf alternating with d."""
    ard = n % 2 == 1
    kind = "Matern52" if d in (1, 16) else "Rbf"
    x = rng.normal(1000 + 31 * n + d, (n, d)) * (1.0 / np.sqrt(d))
    ls = 0.7 + 0.6 * rng.uniform(2000 + n + d, d if ard else 1)
    return kind, ard, x, 1.3, ls


@pytest.mark.parametrize("d", EDGE_D)
@pytest.mark.parametrize("n", EDGE_N)
def test_laplace_system_against_the_scaled_kernel_matrix(device, n, d):
    """B_ij = delta_ij + s_i s_j k_ij with the k_ij bits of gpn_kernel_matrix: three roundings (s_i s_j, times k, plus 1) separate
    it from the host product, so |err| <= 4 * 2^-53 |B_ij|; nothing above the diagonal or in the padding is touched."""
    kind, _, x, var, ls = edge_problem(n, d)
    X, v, l = cuda(x), cuda([var]), cuda(ls)
    s = cuda(0.05 + 2.0 * rng.uniform(3000 + n + d, n))
    ld = int(_native.lib().gpn_factor_ld(n, 1))
    sentinel = -7.25
    A = torch.full((n + 3, ld), sentinel, dtype=torch.float64, device=device)
    _ops.laplace_system(kind, X, v, l, s, A, ld)
    K = _ops.kernel_matrix(kind, X, None, v, l, out=torch.zeros(n, ld, dtype=torch.float64, device=device), ldk=ld, lower=True)[:, :n]
    want = (s[:, None] * s[None, :]).cpu().numpy().astype(np.longdouble) * K.cpu().numpy().astype(np.longdouble) + np.eye(n, dtype=np.longdouble)
    got = A[:n, :n].cpu().numpy()
    low = np.tril(np.ones((n, n), dtype=bool))
    ratio = np.abs(got.astype(np.longdouble) - want)[low] / np.abs(want[low])
    print("system n %d d %d %s: worst err %.2f ulp" % (n, d, kind, float(ratio.max() / U)))
    assert float(ratio.max()) <= 4 * U
    assert np.all(got[~low] == sentinel)
    assert bool((A[:n, n:] == sentinel).all()) and bool((A[n:] == sentinel).all())
    B = torch.full((n + 3, ld), sentinel, dtype=torch.float64, device=device)
    _ops.laplace_system(kind, X, v, l, s, B, ld)
    assert torch.equal(A, B)


def _spd_inverse_like(n, seed):
    """a random SPD matrix standing in for Binv, diagonally dominant enough to be well scaled."""
    g = rng.normal(seed, (n, n + 3))
    return g @ g.T / (n + 3) + 0.5 * np.eye(n)


@pytest.mark.parametrize("d", EDGE_D)
@pytest.mark.parametrize("n", EDGE_N)
def test_laplace_diag_grad_and_matvec_against_long_double(device, n, d):
    kind, ard, x, var, ls = edge_problem(n, d)
    X, v, l = cuda(x), cuda([var]), cuda(ls)
    s = 0.05 + 2.0 * rng.uniform(4000 + n + d, n)
    a, u, d1, vec = (rng.normal(5000 + 7 * k + n + d, (n,)) for k in range(4))
    Binv = _spd_inverse_like(n, 6000 + n + d)
    Bl = cuda(np.tril(Binv) + np.triu(np.full((n, n), np.nan), 1))            # the upper triangle must never be read
    LD = lo.LD
    full_ls = np.asarray(ls if ard else np.full(d, ls[0]))

    def host(dt):
        K = lo.kern(kind, x, None, var, full_ls.astype(dt), dt)[0]
        sd, Bd = s.astype(dt), Binv.astype(dt)
        sigma = np.sum(K * Bd * sd[None, :], 1) / sd
        G = dt(0.5) * (np.outer(a.astype(dt), a.astype(dt)) - sd[:, None] * Bd * sd[None, :] + np.outer(u.astype(dt), d1.astype(dt))
                       + np.outer(d1.astype(dt), u.astype(dt)))
        return K @ vec.astype(dt), sigma, G

    kv64, sig64, G64 = host(np.float64)
    kvld, sigld, Gld = host(LD)
    gv, gl = xr.kernel_param_grads(kind, x, None, var, full_ls, Gld, ard)
    want_g = np.concatenate([gv / LD(var), gl / np.asarray(ls, dtype=LD)])       # w.r.t. the constrained values
    gv64, gl64 = xr.kernel_param_grads(kind, x, None, var, full_ls, G64, ard)    # (long-double sums of the fp64 G: a lower bound of e64)
    e_g = xr.rel_err(np.concatenate([gv64 / LD(var), gl64 / np.asarray(ls, dtype=LD)]), want_g)

    got_kv = _ops.laplace_matvec(kind, X, v, l, cuda(vec))
    got_sig = _ops.laplace_diag(kind, X, v, l, cuda(s), Bl)
    got_g = _ops.laplace_grad(kind, X, v, l, cuda(s), Bl, cuda(a), cuda(u), cuda(d1))
    for name, got, want, e64 in (("matvec", got_kv, kvld, xr.rel_err(kv64, kvld)), ("diag", got_sig, sigld, xr.rel_err(sig64, sigld)),
                                 ("grad", got_g, want_g, e_g)):
        err = xr.rel_err(got, want)
        print("%s n %d d %d %s ard %d: rel err %.2e (e64 %.1e, tol %.1e)" % (name, n, d, kind, ard, err, e64, xr.tol(e64, "dense_grad")))
        assert err <= xr.tol(e64, "dense_grad"), name
    assert torch.equal(got_kv, _ops.laplace_matvec(kind, X, v, l, cuda(vec)))
    assert torch.equal(got_sig, _ops.laplace_diag(kind, X, v, l, cuda(s), Bl))
    assert torch.equal(got_g, _ops.laplace_grad(kind, X, v, l, cuda(s), Bl, cuda(a), cuda(u), cuda(d1)))


# ---- the golden model cases ---------------------------------------------------------------------------------------------------------
def cuda_model(case):
    inp = lo.case_inputs(case)
    m = lo.build_model(case, inp)
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
    print("%s: loss %.12f golden %.12f rel err %.2e (tol %.1e), %s" % (name, loss.item(), case["loss"], err, xr.tol(e["loss"], "loss"), m.newton_stats))
    assert err <= xr.tol(e["loss"], "loss")
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
    mean2, cov = m.predict_f(xs, diag=False)
    ec = xr.abs_err(cov, arr(case, "cov"))
    print("   predict_f: mean %.2e (tol %.1e) var %.2e (tol %.1e) cov %.2e (tol %.1e)"
          % (em, xr.tol(e["mean"], "mean"), ev, xr.tol(e["var"], "var"), ec, xr.tol(e["cov"], "var")))
    assert em <= xr.tol(e["mean"], "mean") and ev <= xr.tol(e["var"], "var") and ec <= xr.tol(e["cov"], "var")
    assert xr.abs_err(mean2[:, 0], arr(case, "mean")) <= xr.tol(e["mean"], "mean")
    # predict_y: the likelihood's own map of the golden marginals.  Its derivatives w.r.t. (mean_f, var_f) are bounded by
    # 2 max(1, |y|) for all three likelihoods (Bernoulli: 0.4 and 0.25; Poisson: E[y] and Var[y] ~ E[y] + 2 (e^v - 1) E[y]^2),
    # so the marginals' tolerances propagate with that factor, plus 64 ulp for the special functions of two libraries
    gm = torch.tensor(arr(case, "mean"))[:, None]
    gvv = torch.tensor(arr(case, "var"))[:, None]
    wy_m, wy_v = m.likelihood.predict_mean_variance(gm, gvv)
    py_m, py_v = m.predict_y(xs)
    for got, want in ((py_m, wy_m), (py_v, wy_v)):
        scale = max(1.0, float(want.abs().max()))
        tol = (4.0 * (xr.tol(e["mean"], "mean") + xr.tol(e["var"], "var")) + 64 * U) * scale
        print("   predict_y: err %.2e tol %.1e" % (xr.abs_err(got, want.numpy()), tol))
        assert xr.abs_err(got, want.numpy()) <= tol
    with pytest.raises(NotImplementedError):
        m.predict_y(xs, diag=False)


def test_warm_and_cold_start_agree(device):
    case = CASES["probit_matern52_ard_513x3"]
    _, m = cuda_model(case)
    with torch.no_grad():
        cold = m.loss()
        cold_stats = dict(m.newton_stats)
        warm = m.loss()
        warm_stats = dict(m.newton_stats)
        m.reset_mode()
        again = m.loss()
    print("cold %.14f %s warm %.14f %s" % (cold.item(), cold_stats, warm.item(), warm_stats))
    assert xr.rel_err(warm.item(), cold.item()) <= xr.tol(case["e64"]["loss"], "loss")
    assert warm_stats["steps"] < cold_stats["steps"]
    assert torch.equal(again, cold) and m.newton_stats == cold_stats


def test_adam_steps_follow_the_oracle(device):
    """optimize(method="Adam", max_iter=10) lowers the loss along the trajectory of torch's CPU Adam on the dense fp64 oracle
    (the bound of the sparse models' trajectory tests: 1e-7 relative)."""
    t = META["trajectory"]
    _, m = cuda_model(CASES[t["case"]])
    with quiet():
        losses, _ = m.optimize(method="Adam", max_iter=t["steps"], learning_rate=t["learning_rate"], verbose=False)
    want = np.asarray(t["losses"])
    err = np.max(np.abs(losses - want) / np.maximum(1.0, np.abs(want)))
    print("laplace adam trajectory: losses %s max rel err %.2e" % (losses, err))
    assert losses[-1] < losses[0] and all(a > b for a, b in zip(losses, losses[1:]))
    assert err < 1e-7


def test_lbfgs_separates_two_clusters(device):
    n, d = 160, 2
    labels = (rng.uniform(41, n) < 0.5).astype(np.float64)
    x = rng.normal(42, (n, d)) * 0.6 + (2.0 * labels[:, None] - 1.0) * 2.0
    train, held = slice(0, 120), slice(120, n)
    m = LaplaceGP(x[train], labels[train, None], kernels.Rbf(d, variance=1.0, length_scales=1.0), likelihoods.Bernoulli("probit"))
    m.cuda()
    with torch.no_grad():
        before = m.loss().item()
    with quiet():
        res = m.optimize(method="L-BFGS-B", max_iter=15, verbose=False)
    with torch.no_grad():
        after = m.loss().item()
    p, v = m.predict_y(x[held])
    print("L-BFGS-B: loss %.6f -> %.6f (%d evaluations)" % (before, after, res.nfev))
    assert after < before
    assert np.array_equal((p[:, 0] > 0.5).astype(np.float64), labels[held])
    assert np.all(v >= 0.0) and np.all(v <= 0.25 + 1e-12)


def test_poisson_case_halves_as_the_oracle(device):
    case = CASES["poisson_rbf_513x2"]
    assert case["halvings"] >= 1
    _, m = cuda_model(case)
    with torch.no_grad():
        m.loss()
    print("poisson halving case: %s, oracle steps %d halvings %d" % (m.newton_stats, case["steps"], case["halvings"]))
    assert m.newton_stats["halvings"] == case["halvings"]
    assert m.newton_stats["steps"] == case["steps"]
