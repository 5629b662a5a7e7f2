"""The non-Gaussian likelihoods on the GPU: gpn_lik_expect (csrc/lik.hip) through the C ABI against the 40-digit goldens of
tests/golden/make_lik_golden.py at 256 * 2^-53 * S (tests/_lik_cases.py: the bound and where it comes from), its determinism
and argument validation, and SVGP with each likelihood: the fused node against the torch route, training, prediction, and the
routes that must stay where they were."""
import contextlib
import ctypes
import io
import math

import numpy as np
import pytest
import torch

from gptorch_amd import _native, _ops, kernels, likelihoods, param, rng, settings
from gptorch_amd.models import SVGP, sparse_gpr
from tests import _lik_cases as lc

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
ROWS = [1, 63, 64, 65, 257, 513, 1000]      # 257: just across a workgroup's share of rows (256), 513: across the second one


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def dev_t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device="cuda")


def call(g, H, c, pad=(0, 0, 0), outs=(True, True, True, True), work_slack=0):
    """gpn_lik_expect on a composed problem `c` of group g -> (status, value, g_mean [rows, dy + pad], g_var, g_params); an
    output that is not asked for is passed as NULL.  pad: extra columns of the f_mean, y and g_mean buffers."""
    rows, dy = c["mu"].shape
    kind = int(lc.GOLD["kind"][g])
    params = dev_t(lc.GOLD["params"][g]) if kind == _native.LIK_STUDENT_T else None
    buf = lambda a, extra: torch.cat([dev_t(a), torch.full((rows, extra), SENTINEL, dtype=torch.float64, device="cuda")], 1).contiguous()
    mu, y, v = buf(c["mu"], pad[0]), buf(c["y"], pad[1]), dev_t(c["v"])
    x, w = dev_t(lc.GOLD["nodes_%d" % H]), dev_t(lc.GOLD["weights_%d" % H])
    blocks = (rows + _native.LIK_ROWS_PER_GROUP - 1) // _native.LIK_ROWS_PER_GROUP
    work = torch.empty(2 * blocks + work_slack, dtype=torch.float64, device="cuda")
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")
    value, g_mean, g_var, g_params = full(1), full(rows, dy + pad[2]), full(rows), full(2)
    ptr = lambda t, on: _ops._ptr(t) if on else None
    st = _native.lib().gpn_lik_expect(_ops._stream(mu.device), kind, _ops._ptr(params), _ops._ptr(mu), mu.stride(0), _ops._ptr(v), _ops._ptr(y),
                                      y.stride(0), rows, dy, _ops._ptr(x), _ops._ptr(w), H, _ops._ptr(work), work.numel() * 8,
                                      ptr(value, outs[0]), ptr(g_mean, outs[1]), g_mean.stride(0), ptr(g_var, outs[2]), ptr(g_params, outs[3]))
    return st, value, g_mean, g_var, g_params


def check_against_golden(g, H, c, res, tag):
    st, value, g_mean, g_var, g_params = res
    assert st == 0
    dy = c["mu"].shape[1]
    ratios = dict(val=lc.worst(value.item(), c["val"], c["val_S"]), dmu=lc.worst(g_mean[:, :dy].cpu().numpy(), c["dmu"], c["dmu_S"]),
                  dv=lc.worst(g_var.cpu().numpy(), c["dv"], c["dv_S"]), dp=lc.worst(g_params[1].item(), c["dp"], c["dp_S"]))
    print("%s H=%d %s: worst |err| / (2^-53 S): %s" % (lc.GROUPS[g], H, tag, {k: round(r, 2) for k, r in ratios.items()}))
    for k, r in ratios.items():
        assert r < 256.0, (tag, k, r)
    assert g_params[0].item() == 0.0
    return ratios


@pytest.mark.parametrize("H", lc.HS)
@pytest.mark.parametrize("g", range(len(lc.GROUPS)), ids=lc.GROUPS)
def test_kernel_meets_the_goldens(device, g, H):
    """value, g_mean, g_var (summed over the row's dy columns) and g_params of every kind and H, at row counts around the
    wavefront and the workgroup's share, dy = 1 and 3, within 256 * 2^-53 * S; a padded leading dimension leaves the padding
    alone and changes no bit."""
    ih = lc.HS.index(H)
    for dy in (1, 3):
        for rows in ROWS:
            check_against_golden(g, H, lc.compose(g, ih, rows, dy), call(g, H, lc.compose(g, ih, rows, dy)), "rows=%d dy=%d" % (rows, dy))
    c = lc.compose(g, ih, 257, 3)
    plain, padded = call(g, H, c), call(g, H, c, pad=(5, 2, 3), work_slack=7)
    check_against_golden(g, H, c, padded, "padded")
    assert torch.equal(padded[1], plain[1]) and torch.equal(padded[2][:, :3], plain[2]) and torch.equal(padded[3], plain[3])
    assert bool((padded[2][:, 3:] == SENTINEL).all())


@pytest.mark.parametrize("g", range(len(lc.GROUPS)), ids=lc.GROUPS)
def test_null_outputs_and_determinism(device, g):
    """every combination of NULL outputs gives the other outputs the bits of the full call and leaves the rest untouched; the
    same call twice gives the same bits."""
    c = lc.compose(g, 1, 1000, 3)
    full = call(g, 20, c)
    again = call(g, 20, c)
    assert full[0] == 0 and all(torch.equal(a, b) for a, b in zip(full[1:], again[1:]))
    for mask in range(16):
        outs = tuple(bool(mask >> b & 1) for b in range(4))
        res = call(g, 20, c, outs=outs)
        assert res[0] == 0
        for on, got, want in zip(outs, res[1:], full[1:]):
            if on:
                assert torch.equal(got, want), (outs,)
            else:
                assert bool((got == SENTINEL).all()), (outs,)


def test_wrapper_matches_the_abi_call(device):
    """_ops.lik_expect: the same bits as the direct call, None for what is not wanted, a row-sliced (strided) f_mean as it is."""
    g = lc.GROUPS.index("student_t_narrow")
    c = lc.compose(g, 1, 300, 3)
    full = call(g, 20, c)
    x, w = dev_t(lc.GOLD["nodes_20"]), dev_t(lc.GOLD["weights_20"])
    wide = torch.cat([dev_t(c["mu"]), torch.zeros(300, 2, dtype=torch.float64, device="cuda")], 1)
    value, g_mean, g_var, g_params = _ops.lik_expect(_native.LIK_STUDENT_T, dev_t(lc.GOLD["params"][g]), wide[:, :3], dev_t(c["v"]), dev_t(c["y"]), x, w)
    assert value.dim() == 0 and torch.equal(value.reshape(1), full[1]) and torch.equal(g_mean, full[2]) and torch.equal(g_var, full[3])
    assert torch.equal(g_params, full[4])
    only = _ops.lik_expect(_native.LIK_STUDENT_T, dev_t(lc.GOLD["params"][g]), wide[:, :3], dev_t(c["v"]), dev_t(c["y"]), x, w, want_mean=False,
                           want_var=False, want_params=False)
    assert only[1] is None and only[2] is None and only[3] is None and torch.equal(only[0], value)
    with pytest.raises(ValueError):
        _ops.lik_expect(_native.LIK_PROBIT, None, wide[:, :3], dev_t(c["v"])[:-1], dev_t(c["y"]), x, w)
    with pytest.raises(_native.NativeError):
        _ops.lik_expect(_native.LIK_PROBIT, None, wide[:, :3].cpu(), dev_t(c["v"]).cpu(), dev_t(c["y"]).cpu(), x.cpu(), w.cpu())


def test_negative_variance_gives_nan(device):
    """v < 0 is not special-cased: NaN for that row's outputs and the value, as the sqrt of the torch route gives."""
    g = lc.GROUPS.index("probit")
    c = lc.compose(g, 1, 65, 1)
    c["v"] = c["v"].copy()
    c["v"][7] = -0.5
    st, value, g_mean, g_var, _ = call(g, 20, c)
    assert st == 0 and math.isnan(value.item()) and math.isnan(g_mean[7, 0].item()) and math.isnan(g_var[7].item())
    keep = np.arange(65) != 7
    assert bool(np.isfinite(g_mean.cpu().numpy()[keep]).all()) and bool(np.isfinite(g_var.cpu().numpy()[keep]).all())


def test_argument_validation_without_launch(device):
    """-(argument index) / GPN_E_* before any HIP call: every pointer here is NULL or a host address that is never read."""
    lib = _native.lib()
    one = (ctypes.c_double * 4)()
    p = ctypes.cast(one, ctypes.c_void_p)
    ok = dict(kind=0, params=None, f_mean=p, ldf=3, f_var=p, y=p, ldy=3, rows=10, dy=3, nodes=p, weights=p, H=20, work=p, work_bytes=16,
              value=None, g_mean=None, ldg=3, g_var=None, g_params=None)

    def status(**kw):
        a = dict(ok, **kw)
        return lib.gpn_lik_expect(None, a["kind"], a["params"], a["f_mean"], a["ldf"], a["f_var"], a["y"], a["ldy"], a["rows"], a["dy"],
                                  a["nodes"], a["weights"], a["H"], a["work"], a["work_bytes"], a["value"], a["g_mean"], a["ldg"],
                                  a["g_var"], a["g_params"])
    assert status(kind=4) == -2 and status(kind=-1) == -2
    assert status(kind=_native.LIK_STUDENT_T) == -3            # Student-t without (df, scale^2)
    assert status(f_mean=None) == -4
    assert status(ldf=2) == -5
    assert status(f_var=None) == -6
    assert status(y=None) == -7
    assert status(ldy=2) == -8
    assert status(rows=0) == -9
    assert status(dy=0) == -10
    assert status(nodes=None) == -11
    assert status(weights=None) == -12
    assert status(H=0) == -13 and status(H=65) == -13
    assert status(work=None) == -14
    assert status(work_bytes=8) == -15 and status(rows=257, work_bytes=16) == -15
    assert status(g_mean=p, ldg=2) == -18
    assert status(kind=_native.LIK_POISSON, nodes=None, weights=None, H=0, work=None) == -14   # Poisson reads no rule
    assert lib.gpn_last_hip_error() == b""


def make_data(name, n, seed):
    x, f = rng.make_regression(n, 2, 1, seed=seed)
    if name in ("probit", "logit"):
        y = (f > 0.1).astype(np.float64)
    elif name == "poisson":
        y = np.floor(np.exp(1.0 + f))
    else:
        y = f.copy()
        y[::17] += 8.0                                           # outliers
    return x, y


def make_model(name, batch_size=None, n=300, m=24, seed=5):
    lik = {"probit": lambda: likelihoods.Bernoulli(), "logit": lambda: likelihoods.Bernoulli(link="logit"),
           "poisson": likelihoods.Poisson, "student_t": lambda: likelihoods.StudentT(df=4.0, scale=0.6)}[name]()
    x, y = make_data(name, n, seed)
    np.random.seed(3)
    model = SVGP(x, y, kernels.Rbf(2), num_inducing_points=m, likelihood=lik, batch_size=batch_size)
    model.cuda()
    return model


@pytest.mark.parametrize("batch_size", [None, 64], ids=["full", "batch64"])
@pytest.mark.parametrize("name", ["probit", "logit", "poisson", "student_t"])
def test_model_native_route_equals_torch_route(device, monkeypatch, name, batch_size):
    """SVGP (N = 300, d = 2, M = 24, dy = 1): loss and gradients with NATIVE_EXPECTATION on and off, the same host draw for the
    minibatch: values to 1e-12 relative (test_gaussian_shortcut_equals_generic_route), gradients per parameter block to
    1e-7 x max |gradient| with the torch route as the reference (check_grads of tests/test_gpu_svgp.py)."""
    m = make_model(name, batch_size)
    calls = []
    real = _ops.lik_expect
    monkeypatch.setattr(_ops, "lik_expect", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    out = []
    for flag in (True, False):
        monkeypatch.setattr(sparse_gpr, "NATIVE_EXPECTATION", flag)
        m.zero_grad()
        np.random.seed(11)
        loss = m.loss()
        loss.backward()
        assert len(calls) == 1                                   # on: one call per evaluation; off: none
        out.append((loss.item(), {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters() if p.grad is not None}))
    (got, got_g), (want, want_g) = out
    print("%s %s: native %.15g torch %.15g" % (name, batch_size, got, want))
    assert math.isfinite(want) and abs(got - want) < 1e-12 * abs(want)
    assert set(got_g) == set(want_g) and len(want_g) >= 5 + (name == "student_t")
    for n, gw in want_g.items():
        scale = float(np.max(np.abs(gw)))
        err = float(np.max(np.abs(got_g[n] - gw)))
        print("   d/d%-32s err %.2e of max %.2e" % (n, err, scale))
        assert err < 1e-7 * scale, (n, err, scale)


def test_bernoulli_probit_trains_and_predicts(device):
    """labels x_0 > 0 on 400 points: three full-batch Adam steps lower the loss each time (test_custom_likelihood_trains);
    predict_y gives probabilities with variance p (1 - p); the Gaussian-only routes raise."""
    x, _ = rng.make_regression(400, 2, 1, seed=5)
    y = (x[:, :1] > 0.0).astype(np.float64)
    np.random.seed(3)
    m = SVGP(x, y, kernels.Rbf(2), num_inducing_points=20, likelihood=likelihoods.Bernoulli())
    m.cuda()
    with quiet():
        losses, _ = m.optimize(method="Adam", max_iter=3, verbose=False)
    print("bernoulli losses", losses)
    assert losses[0] > losses[1] > losses[2]
    xs = np.stack([np.linspace(-2.0, 2.0, 9), np.zeros(9)], 1)
    p, var = m.predict_y(xs)
    assert p.shape == (9, 1) and var.shape == (9, 1)
    assert np.all((p >= 0.0) & (p <= 1.0)) and np.allclose(var, p * (1.0 - p), rtol=0, atol=1e-15)
    assert p[-1, 0] > p[0, 0]                                     # the side of the labels
    with pytest.raises(NotImplementedError):
        m.predict_y(xs, diag=False)
    with pytest.raises(NotImplementedError):
        m.predict_y_samples(xs, n_samples=2)


class ScaledGaussian(likelihoods.Likelihood):
    """a user likelihood with its own propagate_log (as tests/test_gpu_svgp.py's)."""

    def __init__(self, scale=2.0):
        super().__init__()
        self.scale = scale
        self.variance = param.Param(torch.tensor([0.2], dtype=torch.float64), transform=settings.DefaultPositiveTransform())

    def propagate_log(self, qf, targets):
        s2 = self.scale * self.variance.transform()
        return -0.5 * (targets.nelement() * (math.log(2.0 * math.pi) + torch.log(s2))
                       + (torch.sum((targets - qf.loc) ** 2) + qf.variance.sum()) / s2)


class MyBernoulli(likelihoods.Bernoulli):
    """a subclass may override logp: it keeps the torch route."""


def test_other_likelihoods_keep_their_routes(device, monkeypatch):
    """Gaussian, a user likelihood and a SUBCLASS of a native class never reach the native entry point."""
    def refuse(*a, **k):
        raise AssertionError("gpn_lik_expect must not be called")
    monkeypatch.setattr(_ops, "lik_expect", refuse)
    x, y = rng.make_regression(200, 2, 1, seed=5)
    for lik, yy in ((ScaledGaussian(), y), (likelihoods.Gaussian(variance=0.3), y), (MyBernoulli(), (y > 0).astype(np.float64))):
        np.random.seed(3)
        m = SVGP(x, yy, kernels.Rbf(2), num_inducing_points=12, likelihood=lik)
        m.cuda()
        loss = m.loss()
        loss.backward()
        assert math.isfinite(loss.item())
    np.random.seed(3)
    m = SVGP(x, (y > 0).astype(np.float64), kernels.Rbf(2), num_inducing_points=12, likelihood=likelihoods.Bernoulli())
    m.cuda()
    with pytest.raises(AssertionError, match="must not be called"):
        m.loss()
