"""Every stationary kind -- Rbf, Matern52, Matern32, Exp (and its alias Matern12), Periodic -- through the native path
against the extended-precision reference of tests/_xref.py: kernel assembly (kmat.hip), the dense-mode and point gradient
sweeps (grad.hip) on both sides of each register / chunked variant, GPR's loss, gradients and predictions, the refined LML
(refine.hip) and VFE.  Every check is held to xr.tol: 16 x the error of a plain fp64 CPU evaluation of the same quantity
(direct-difference distances), floored (tests/_xref.py).  The Gram-trick oracle cannot judge Exp at this level: its own
values are ~1e-8 off (tests/test_xref.py::test_the_oracle_fails_the_exp_tolerance).

Periodic (var cos r, Euclidean r) is indefinite for d >= 2: its GPR cases run at d = 1 (rank-2 K) or with a noise variance
above |lambda_min(K)|."""
import math

import numpy as np
import pytest
import torch

from gptorch_amd import kernels, likelihoods, mean_functions, rng
from gptorch_amd.models import GPR, VFE
from oracle import gp_oracle as orc
from tests import _xref as xr
from tests._refine_ref import points as _points        # the planted rows (shared with the refinement's tests)

pytestmark = pytest.mark.gpu

KERN = {"Rbf": kernels.Rbf, "Matern52": kernels.Matern52, "Matern32": kernels.Matern32, "Exp": kernels.Exp,
        "Matern12": kernels.Matern12, "Periodic": kernels.Periodic}
VAR = 1.3


def _t(a, device=None, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=device, requires_grad=grad)


def _ls(d, ard, seed, scale):
    return scale * (0.6 + 0.8 * rng.uniform(seed, d)) if ard else float(scale)


def _direct64(kind, xn, x2n, ls, wn):
    """fp64 CPU evaluation by direct differences: K, d sum(W K)/d(log var, log ell) (autograd)."""
    rv = _t([math.log(VAR)], grad=True)
    rl = _t(np.log(np.atleast_1d(ls)), grad=True)
    Kd = xr.direct_kernel_K(kind, _t(xn), None if x2n is None else _t(x2n), rv.exp(), rl.exp())
    (Kd * _t(wn)).sum().backward()
    return Kd.detach(), rv.grad, rl.grad


# ---- kernel assembly and the dense-mode hyper-parameter sweep ---------------------------------------------------------
SHAPES = [(1, 1, 1), (63, 65, 15), (64, 64, 16), (65, 63, 17), (128, 129, 48), (129, 128, 49), (257, 64, 64), (65, 257, 65)]


@pytest.mark.parametrize("kind", xr.KINDS)
@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("n,m,d", SHAPES)
def test_kernel_matrix_and_dense_gradients(device, kind, ard, n, m, d):
    """Kernel.K(X), K(X, X2), Kdiag (kmat.hip) and d sum(W K)/d(log variance, log ell) (gpn_kernel_grad, dense mode: 16 / 32 /
    48 / 64 coordinates in registers, the chunked kernel above) -- with repeated, near-repeated, far and Periodic-edge rows in
    both sets, and X2 sharing rows with X."""
    ls = _ls(d, ard, 40 + d, 0.8 * math.sqrt(d))
    ls0 = float(np.atleast_1d(ls)[0])
    xn = _points(n + 7 * d, n, d, ls0)
    x2n = _points(m + 11 * d, m, d, ls0, first=3)
    k2 = min(n, len(range(1, m, 5)))
    x2n[1:5 * k2:5] = xn[:k2]
    k = KERN[kind](d, variance=VAR, length_scales=ls, ARD=ard)
    k.cuda()
    X, X2 = _t(xn, device), _t(x2n, device)
    for other, wseed in ((None, 1), (x2n, 2)):
        wn = rng.normal(100 * d + n + wseed, (n, n if other is None else m))
        k.zero_grad()
        Kg = k.K(X, None if other is None else X2)
        (Kg * _t(wn, device)).sum().backward()
        Kr = xr.K(kind, xn, other, VAR, ls)
        gv, gl = xr.kernel_param_grads(kind, xn, other, VAR, ls, wn, ard)
        K64, gv64, gl64 = _direct64(kind, xn, other, ls, wn)
        Kg = Kg.detach().cpu()
        assert xr.abs_err(Kg, Kr) <= xr.tol(xr.abs_err(K64, Kr), "K"), (xr.abs_err(Kg, Kr), xr.abs_err(K64, Kr))
        e64 = max(xr.rel_err(gv64, gv), xr.rel_err(gl64, gl))
        err = max(xr.rel_err(k.variance.grad.cpu(), gv), xr.rel_err(k.length_scales.grad.cpu(), gl))
        assert err <= xr.tol(e64, "dense_grad"), (err, e64)
        if other is None:
            assert torch.equal(Kg, Kg.t())
            assert torch.all(Kg.diagonal() == VAR)          # Exp too: its cusp is exact with direct differences
    assert torch.all(k.Kdiag(X).cpu() == VAR)


# ---- gradients w.r.t. the points (gpn_kernel_grad_x2) -----------------------------------------------------------------
@pytest.mark.parametrize("kind", xr.KINDS)
@pytest.mark.parametrize("n,m,d,ard", [(64, 65, 16, True), (65, 64, 17, False), (129, 63, 33, True), (63, 129, 64, False),
                                       (130, 66, 65, True)])
def test_point_gradients(device, kind, n, m, d, ard):
    """d sum(W K(X, X2))/dX, /dX2 and d sum(W K(X))/dX: the register kernels (d <= 16, 32, 64) and the chunked one above.  Where
    every weight sits on pairs at distance 0 or under the clamp, the gradient is exactly 0 for every kind."""
    ls = _ls(d, ard, 50 + d, 0.8 * math.sqrt(d))
    ls0 = float(np.atleast_1d(ls)[0])
    xn = _points(n + 3 * d, n, d, ls0)
    x2n = _points(m + 5 * d, m, d, ls0, first=2)
    x2n[4::6] = xn[:len(x2n[4::6])]
    wn, wsn = rng.normal(60 + d, (n, m)), rng.normal(61 + d, (n, n))
    k = KERN[kind](d, variance=VAR, length_scales=ls, ARD=ard)
    k.cuda()
    X, X2, Xs = _t(xn, device, True), _t(x2n, device, True), _t(xn, device, True)
    (k.K(X, X2) * _t(wn, device)).sum().backward()
    (k.K(Xs) * _t(wsn, device)).sum().backward()
    gX, gX2 = xr.kernel_point_grads(kind, xn, x2n, VAR, ls, wn)
    gXs = xr.kernel_point_grads(kind, xn, None, VAR, ls, wsn)
    lso = _t(np.atleast_1d(ls))
    Xo, X2o, Xso = _t(xn, grad=True), _t(x2n, grad=True), _t(xn, grad=True)
    (xr.direct_kernel_K(kind, Xo, X2o, _t([VAR]), lso) * _t(wn)).sum().backward()
    (xr.direct_kernel_K(kind, Xso, None, _t([VAR]), lso) * _t(wsn)).sum().backward()
    for got, g64, want in [(X.grad, Xo.grad, gX), (X2.grad, X2o.grad, gX2), (Xs.grad, Xso.grad, gXs)]:
        err, e64 = xr.rel_err(got.cpu(), want), xr.rel_err(g64, want)
        assert err <= xr.tol(e64, "point_grad"), (err, e64)
    # weights only on exactly repeated pairs -- and for the clamped kinds on every pair under the clamp (kernels.py:172):
    # no gradient at all
    r2 = xr.scaled_sqdist(xn, None, ls)
    wz = np.where(r2 == 0 if kind == "Rbf" else r2 < xr.CLAMP, wsn, 0.0)
    assert np.count_nonzero(wz) > n                     # the planted pairs, not just the diagonal
    Xz = _t(xn, device, True)
    (k.K(Xz) * _t(wz, device)).sum().backward()
    assert torch.count_nonzero(Xz.grad) == 0


# ---- GPR: loss, gradients, predictions --------------------------------------------------------------------------------
# (name, kind, n, d, dy, ard, noise: a number or "pd" = 1.5 |lambda_min(K)| + 0.05, gradients checked, special rows)
GPR_CASES = [
    ("exp_1", "Exp", 1, 3, 1, False, 0.05, True, False),
    ("exp_2_ard", "Exp", 2, 2, 4, True, 0.05, True, False),
    ("m12_64", "Matern12", 64, 3, 5, False, 0.05, True, False),
    ("exp_65_ard", "Exp", 65, 5, 9, True, 0.02, True, False),
    ("per1_127", "Periodic", 127, 1, 4, False, 0.05, True, False),
    ("exp_129_ard", "Exp", 129, 8, 1, True, 0.05, True, False),
    ("per1_257_ard", "Periodic", 257, 1, 5, True, 0.1, True, False),
    ("exp_300_table", "Exp", 300, 3, 1, False, 0.05, True, False),
    ("m12_513", "Matern12", 513, 3, 9, False, 0.05, True, False),
    ("exp_rep_200", "Exp", 200, 3, 2, True, 0.05, True, True),
    ("per17_65_ard", "Periodic", 65, 17, 1, True, "pd", True, False),
    ("per64_129", "Periodic", 129, 64, 5, False, "pd", True, False),
    ("rbf49_257_ard", "Rbf", 257, 49, 5, True, 0.05, True, False),
    ("m52_64_129", "Matern52", 129, 64, 9, False, 0.05, True, False),
    ("m52_64_200_ard", "Matern52", 200, 64, 4, True, 0.05, True, False),
    ("m32_56_300_ard", "Matern32", 300, 56, 4, True, 0.05, True, False),
    ("m32_49_129", "Matern32", 129, 49, 1, False, 0.05, True, False),
    ("rbf64_65", "Rbf", 65, 64, 1, False, 0.05, True, False),
    ("exp_1025_ard", "Exp", 1025, 4, 5, True, 0.05, False, False),
    ("per1_1025", "Periodic", 1025, 1, 1, False, 0.05, False, False),
]


def _case_data(c):
    name, kind, n, d, dy, ard, noise, grads, special = c
    x, y = rng.make_regression(n, d, dy, seed=n + d)
    if name == "exp_300_table":
        x = 3.0 * x                                      # spread like the sensitivity check of tests/test_xref.py
    ls = _ls(d, ard, 70 + d, (1.5 if d == 1 else 0.9 * math.sqrt(d)))
    if special:
        ls0 = float(np.atleast_1d(ls)[0])
        x[10:20] = x[:10]                                # repeated rows, near-repeated rows (r ~ 1e-9) ...
        x[20:30] = x[:10] + 1e-9 * ls0
        x[30:34] = 0.0                                   # ... and pairs at r = 1e-21 (under the clamp), 1e-19, 1e-12
        x[31:34, 0] = np.array([1e-21, 1e-19, 1e-12]) * ls0
    mean = np.linspace(-0.3, 0.25, dy)
    xs = np.concatenate([rng.normal(n + 99, (12, d)), x[:min(n, 4)], 60.0 * np.max(np.atleast_1d(ls)) * np.ones((2, d))])
    return x, y, ls, mean, xs


def _gpr_reference(c):
    """-> (data, long-double reference values, fp64 direct-difference values) of one case."""
    name, kind, n, d, dy, ard, noise, grads, special = c
    x, y, ls, mean, xs = _case_data(c)
    if noise == "pd":
        lam = np.linalg.eigvalsh(xr.K(kind, x, None, VAR, ls).astype(np.float64)).min()
        assert lam < 0                                   # indefinite: the point of the case
        noise = 1.5 * abs(lam) + 0.05
    r = xr.GPRRef(x, y, kind, VAR, ls, noise, ARD=ard, mean=mean)     # raises unless Kyy is positive definite
    dg = xr.DirectGPR(x, y, kind=kind, variance=VAR, length_scales=ls, noise=noise, ARD=ard, mean=mean)
    ref = {"loss": r.loss()}
    l64, g64 = dg.loss_grads_with_mean()
    d64 = {"loss": l64.item()}
    if grads:
        ref["grads"], d64["grads"] = r.loss_grads(), g64
    with torch.no_grad():
        for f in ("predict_f", "predict_y"):
            for diag in (True, False):
                ref[f, diag] = getattr(r, f)(xs, diag)
                d64[f, diag] = getattr(dg, f)(xs, diag)
    return dict(x=x, y=y, ls=ls, mean=mean, xs=xs, noise=noise), ref, d64


@pytest.fixture(scope="module")
def gpr_refs():
    """each case's references, computed once per module (the refinement test reuses the GPR cases')."""
    cache = {}

    def get(c):
        if c[0] not in cache:
            cache[c[0]] = _gpr_reference(c)
        return cache[c[0]]
    return get


def _gpr_model(c, data, device):
    name, kind, n, d, dy, ard = c[:6]
    mean = mean_functions.Constant(dy, val=torch.tensor(data["mean"], dtype=torch.float64))
    m = GPR(data["x"], data["y"], KERN[kind](d, variance=VAR, length_scales=data["ls"], ARD=ard),
            likelihood=likelihoods.Gaussian(variance=data["noise"]), mean_function=mean)
    m.cuda()
    return m, mean


@pytest.mark.parametrize("c", GPR_CASES, ids=[c[0] for c in GPR_CASES])
def test_gpr_loss_gradients_and_predictions(device, gpr_refs, c):
    """loss() (gpr.py:47-67), the gradients of log variance, log ell, log noise and a trainable Constant mean (the LML-mode
    sweep of grad.hip: dy = 1, 4, 5, 9 right-hand sides against its 4-at-a-time staging), predict_f / predict_y with diag
    True and False at random points, at training points (Exp's cusp in K(x, x*)) and far away (every exp underflows)."""
    data, ref, d64 = gpr_refs(c)
    m, mean = _gpr_model(c, data, device)
    loss = m.loss()
    loss.backward()
    err, e64 = xr.rel_err(loss.item(), ref["loss"]), xr.rel_err(d64["loss"], ref["loss"])
    assert err <= xr.tol(e64, "loss"), ("loss", err, e64)
    if "grads" in ref:
        got = [m.kernel.variance.grad, m.kernel.length_scales.grad, m.likelihood.variance.grad, mean.val.grad]
        for what, g, g64, want in zip(("variance", "ell", "noise", "mean"), got, d64["grads"], ref["grads"]):
            err, e64 = xr.rel_err(g.cpu(), want), xr.rel_err(g64, want)
            assert err <= xr.tol(e64, "grad"), (what, err, e64)
    for f in ("predict_f", "predict_y"):
        for diag in (True, False):
            mu, v = getattr(m, f)(data["xs"], diag=diag)
            for what, got, g64, want in (("mean", mu, d64[f, diag][0], ref[f, diag][0]), ("var", v, d64[f, diag][1], ref[f, diag][1])):
                assert np.shape(got) == np.shape(want)
                err, e64 = xr.abs_err(got, want), xr.abs_err(g64, want)
                assert err <= xr.tol(e64, what), (f, diag, what, err, e64)


# ---- the refined LML (gpn_lml_refine) ---------------------------------------------------------------------------------
REFINE_CASES = [("exp_1025_ard", "Exp", 1025, 4, 5, True, 0.05, False, False),
                ("per1_1153", "Periodic", 1153, 1, 2, False, 0.05, False, False),
                ("m32_1089", "Matern32", 1089, 3, 1, False, 0.02, False, False)]


@pytest.mark.parametrize("c", REFINE_CASES, ids=[c[0] for c in REFINE_CASES])
def test_refined_lml(device, gpr_refs, monkeypatch, c):
    """from refine_min_n() rows on the LML's quadratic form is refined by a residual pass that re-computes Kyy per kind
    (refine.hip): lowered here so that the pass runs for Exp, Periodic and Matern32; refined and plain values both meet the
    tolerance."""
    data, ref, d64 = gpr_refs(c)
    tol = xr.tol(xr.rel_err(d64["loss"], ref["loss"]), "loss")
    for min_n, refined in (("1000", True), ("0", False)):
        monkeypatch.setenv("GPN_REFINE_MIN_N", min_n)
        m, _ = _gpr_model(c, data, device)
        with torch.no_grad():
            lml = m.log_likelihood().item()
        assert m._holder["factor"].refined == refined
        err = xr.rel_err(-lml, ref["loss"])
        assert err <= tol, (min_n, err, tol)


# ---- VFE with Exp (Kuf holds the cusp: inducing points equal to training rows) ----------------------------------------
@pytest.mark.parametrize("n,m,d,dy,ard", [(300, 40, 1, 1, False), (1000, 128, 3, 2, True)])
def test_vfe_exp(device, n, m, d, dy, ard):
    """the collapsed bound (sparse_gpr.py:108-153), its gradients incl. the inducing points and predict_f against DirectVFE,
    at the tolerances of the VFE sweep (tests/sweeps/fuzz_vfe.py)."""
    x, y = rng.make_regression(n, d, dy, seed=n + m)
    z = np.concatenate([x[:m // 4], rng.normal(n + m + 1, (m - m // 4, d))])
    ls = _ls(d, ard, 90 + d, 0.6 * math.sqrt(d))
    noise = 0.05
    mod = VFE(x, y, kernels.Exp(d, variance=VAR, length_scales=ls, ARD=ard), inducing_points=z,
              likelihood=likelihoods.Gaussian(variance=noise), mean_function=mean_functions.Zero(dy))
    mod.cuda()
    o = xr.DirectVFE(x, y, z, "Exp", VAR, ls, noise)
    cond = torch.linalg.cond(o.K(o.Z)).item()
    assert cond < 1e10
    ref = orc.vfe_grads_autograd(o)
    elbo = o.log_likelihood().item()
    mod.zero_grad()
    loss = mod.loss()
    loss.backward()
    assert abs(-loss.item() - elbo) <= 1e-8 * max(1.0, cond * 1e-8) * max(1.0, abs(elbo))
    got = [mod.kernel.variance.grad.cpu().numpy().ravel() / -VAR,
           mod.kernel.length_scales.grad.cpu().numpy().ravel() / -np.atleast_1d(ls),
           mod.likelihood.variance.grad.cpu().numpy().ravel() / -noise, -mod.Z.grad.cpu().numpy()]
    for g, r in zip(got, ref):
        assert np.abs(g.reshape(r.shape) - r.numpy()).max() <= 1e-7 * max(1.0, cond * 1e-6) * max(1.0, np.abs(r.numpy()).max())
    xs = np.concatenate([rng.normal(n + 5, (6, d)), z[:3]])
    for diag in (True, False):
        mu, v = mod.predict_f(xs, diag=diag)
        with torch.no_grad():
            omu, ov = o.predict_f(xs, diag=diag)
        assert np.abs(mu - omu.numpy()).max() <= 1e-6 and np.abs(v - ov.numpy()).max() <= 1e-6
