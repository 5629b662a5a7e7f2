"""likelihoods.MultiClass on the GPU: gpn_lik_expect_robustmax and gpn_lik_robustmax_probs (csrc/multiclass.hip) through the C ABI
against the 40-digit goldens of tests/golden/make_multiclass_golden.py, their determinism, NULL outputs, bad labels and padding,
and SVGP with the likelihood: the fused node against the torch route of the same model, prediction, training.

Tolerances.  Per entry |err| <= max(16 e64, 64 * 2^-53 |golden|), e64 the error of the oracle's plain-fp64 statement (the rule of
tests/test_gpu_laplace.py).  The summed value: the rows' tolerances plus depth * 2^-53 sum |row values|, depth = 2 (the four
rows of a workgroup) + ceil(workgroups / 256) (a thread's sequential share in the second launch) + 8 (its shuffle tree and four
wavefronts).  Model checks: tests/_xref.tol(e64, ...) with e64 from the generator's fp64-against-mpmath evaluation of the same
data term."""
import contextlib
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gptorch_amd import _native, _ops, kernels, likelihoods
from gptorch_amd.models import SVGP, sparse_gpr
from tests import _multiclass_oracle as mo
from tests import _svgp_oracle as so
from tests import _xref as xr
from tests._util import ROOT, load_npz

pytestmark = pytest.mark.gpu

GOLD = load_npz("multiclass_cases.npz")
META = json.loads(str(GOLD["meta"]))
EPS = META["eps"]
U = 2.0 ** -53
SENTINEL = -7.25
ROWS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000]     # around a workgroup's four rows, a wavefront's lanes, the second launch's 256
G = _native.ROBUSTMAX_ROWS_PER_GROUP


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def dev_t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device="cuda")


def deal(C, rows):
    npts = GOLD["C%d_v" % C].size
    return (np.arange(rows) * 7 + rows) % npts                # the golden points, dealt over the rows


def rule(H):
    x, w = np.polynomial.hermite.hermgauss(H)
    return dev_t(x), dev_t(w)


def padded(a, extra):
    a = dev_t(a)
    return torch.cat([a, torch.full((a.shape[0], extra), SENTINEL, dtype=torch.float64, device="cuda")], 1).contiguous()


def call_expect(mu, v, lab, H, pad=(3, 2), outs=(True, True, True), work_slack=0):
    """gpn_lik_expect_robustmax -> (status, value [1], g_mean [rows, C + pad], g_var [rows]); ldf = C + pad[0], ldg = C + pad[1];
    an output that is not asked for is passed as NULL and keeps its sentinels."""
    rows, C = mu.shape
    fm, fv, lb = padded(mu, pad[0]), dev_t(v), dev_t(lab)
    x, w = rule(H)
    work = torch.empty((rows + G - 1) // G + work_slack, dtype=torch.float64, device="cuda")
    full = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")
    value, g_mean, g_var = full(1), full(rows, C + pad[1]), full(rows)
    ptr = lambda t, on: _ops._ptr(t) if on else None
    st = _native.lib().gpn_lik_expect_robustmax(_ops._stream(fm.device), _ops._ptr(fm), fm.stride(0), _ops._ptr(fv), _ops._ptr(lb), rows, C, EPS,
                                                _ops._ptr(x), _ops._ptr(w), H, _ops._ptr(work), work.numel() * 8, ptr(value, outs[0]),
                                                ptr(g_mean, outs[1]), g_mean.stride(0), ptr(g_var, outs[2]))
    return st, value, g_mean, g_var


def call_probs(mu, v, H, pad=(3, 1)):
    rows, C = mu.shape
    fm, fv = padded(mu, pad[0]), dev_t(v)
    x, w = rule(H)
    probs = torch.full((rows, C + pad[1]), SENTINEL, dtype=torch.float64, device="cuda")
    st = _native.lib().gpn_lik_robustmax_probs(_ops._stream(fm.device), _ops._ptr(fm), fm.stride(0), _ops._ptr(fv), rows, C, EPS, _ops._ptr(x),
                                               _ops._ptr(w), H, _ops._ptr(probs), probs.stride(0))
    return st, probs


def entries_ok(C, H, key, idx, got, tag):
    gold, e64 = GOLD["C%d_H%d_%s" % (C, H, key)][idx], GOLD["C%d_H%d_%s_e64" % (C, H, key)][idx]
    err, tol = np.abs(got - gold), np.maximum(16.0 * e64, 64.0 * U * np.abs(gold))
    ratio = err / np.maximum(tol, 1e-300)
    print("C=%d H=%d %s %s: worst err / tol %.3f" % (C, H, tag, key, float(np.max(ratio))))
    assert np.all(err <= tol), (key, tag, int(np.argmax(ratio)), float(np.max(ratio)))


@pytest.mark.parametrize("H", mo.HS)
@pytest.mark.parametrize("C", mo.CLASSES)
def test_entry_points_meet_the_goldens(device, C, H):
    """g_mean, g_var and the probabilities per entry, the summed value, at every row count, with ldf, ldg, ldp > C: the padding
    keeps its sentinels."""
    MU, V, LAB = GOLD["C%d_mu" % C], GOLD["C%d_v" % C], GOLD["C%d_label" % C]
    for rows in ROWS:
        idx = deal(C, rows)
        st, value, g_mean, g_var = call_expect(MU[idx], V[idx], LAB[idx], H)
        assert st == 0
        tag = "rows=%d" % rows
        entries_ok(C, H, "gm", idx, g_mean[:, :C].cpu().numpy(), tag)
        entries_ok(C, H, "gv", idx, g_var.cpu().numpy(), tag)
        assert bool((g_mean[:, C:] == SENTINEL).all())
        val, e64 = GOLD["C%d_H%d_val" % (C, H)][idx], GOLD["C%d_H%d_val_e64" % (C, H)][idx]
        blocks = (rows + G - 1) // G
        depth = 2 + (blocks + 255) // 256 + 8
        tol = float(np.sum(np.maximum(16.0 * e64, 64.0 * U * np.abs(val))) + depth * U * np.sum(np.abs(val)))
        want = float(np.sum(val.astype(np.longdouble)))
        print("C=%d H=%d %s value: err %.3e tol %.3e" % (C, H, tag, abs(value.item() - want), tol))
        assert abs(value.item() - want) <= tol
        st, probs = call_probs(MU[idx], V[idx], H)
        assert st == 0
        entries_ok(C, H, "probs", idx, probs[:, :C].cpu().numpy(), tag)
        assert bool((probs[:, C:] == SENTINEL).all())


@pytest.mark.parametrize("C, H, rows", [(10, 20, 257), (65, 64, 65), (2, 1, 5)])
def test_null_outputs_padding_and_determinism(device, C, H, rows):
    """every combination of NULL outputs gives the others the bits of the full call and writes nothing else; another leading
    dimension and a larger workspace change no bit; the same call twice gives the same bits."""
    idx = deal(C, rows)
    mu, v, lab = GOLD["C%d_mu" % C][idx], GOLD["C%d_v" % C][idx], GOLD["C%d_label" % C][idx]
    full = call_expect(mu, v, lab, H)
    again = call_expect(mu, v, lab, H)
    assert full[0] == 0 and all(torch.equal(a, b) for a, b in zip(full[1:], again[1:]))
    tight = call_expect(mu, v, lab, H, pad=(0, 0), work_slack=5)
    assert torch.equal(tight[1], full[1]) and torch.equal(tight[2], full[2][:, :C]) and torch.equal(tight[3], full[3])
    for mask in range(8):
        outs = tuple(bool(mask >> b & 1) for b in range(3))
        res = call_expect(mu, v, lab, H, outs=outs)
        assert res[0] == 0
        for on, got, want in zip(outs, res[1:], full[1:]):
            assert torch.equal(got, want) if on else bool((got == SENTINEL).all()), (outs,)
    p0, p1 = call_probs(mu, v, H), call_probs(mu, v, H, pad=(0, 0))
    assert p0[0] == 0 and torch.equal(p0[1][:, :C], p1[1]) and torch.equal(call_probs(mu, v, H)[1], p0[1])


def test_a_bad_label_or_variance_gives_nan_in_that_row_only(device):
    C, H, rows = 10, 20, 65
    idx = deal(C, rows)
    mu, v, lab = GOLD["C%d_mu" % C][idx], GOLD["C%d_v" % C][idx].copy(), GOLD["C%d_label" % C][idx].copy()
    clean = call_expect(mu, v, lab, H)
    bad = {3: float(C), 17: -1.0, 30: 1.5, 44: float("nan"), 64: 1.0e300}
    for r, value in bad.items():
        lab[r] = value
    v[9], v[50] = 0.0, -0.5
    st, value, g_mean, g_var = call_expect(mu, v, lab, H)
    assert st == 0 and math.isnan(value.item())
    hit = np.zeros(rows, dtype=bool)
    hit[list(bad) + [9, 50]] = True
    gm, gv = g_mean[:, :C].cpu().numpy(), g_var.cpu().numpy()
    assert np.all(np.isnan(gm[hit])) and np.all(np.isnan(gv[hit]))
    assert np.array_equal(gm[~hit], clean[2][:, :C].cpu().numpy()[~hit]) and np.array_equal(gv[~hit], clean[3].cpu().numpy()[~hit])
    assert bool((g_mean[:, C:] == SENTINEL).all())
    st, probs = call_probs(mu, v, H)
    pr = probs[:, :C].cpu().numpy()
    assert st == 0 and np.all(np.isnan(pr[[9, 50]])) and np.all(np.isfinite(np.delete(pr, [9, 50], 0)))


def test_wrappers_match_the_abi_calls(device):
    C, H, rows = 3, 20, 300
    idx = deal(C, rows)
    mu, v, lab = GOLD["C%d_mu" % C][idx], GOLD["C%d_v" % C][idx], GOLD["C%d_label" % C][idx]
    full = call_expect(mu, v, lab, H, pad=(0, 0))
    x, w = rule(H)
    wide = padded(mu, 2)
    value, g_mean, g_var = _ops.lik_expect_robustmax(wide[:, :C], dev_t(v), dev_t(lab), EPS, x, w)
    assert value.dim() == 0 and torch.equal(value.reshape(1), full[1]) and torch.equal(g_mean, full[2]) and torch.equal(g_var, full[3])
    only = _ops.lik_expect_robustmax(wide[:, :C], dev_t(v), dev_t(lab), EPS, x, w, want_mean=False, want_var=False)
    assert only[1] is None and only[2] is None and torch.equal(only[0], value)
    assert torch.equal(_ops.lik_robustmax_probs(wide[:, :C], dev_t(v), EPS, x, w), call_probs(mu, v, H, pad=(0, 0))[1])
    with pytest.raises(ValueError):
        _ops.lik_expect_robustmax(wide[:, :C], dev_t(v)[:-1], dev_t(lab), EPS, x, w)
    with pytest.raises(_native.NativeError):
        _ops.lik_robustmax_probs(wide[:, :C].cpu(), dev_t(v).cpu(), EPS, x.cpu(), w.cpu())
    # the likelihood's own methods on the GPU are these entry points; with the switch off, the torch route on the same device
    lik = likelihoods.MultiClass(C, EPS)
    assert torch.equal(lik.variational_expectation(dev_t(mu), dev_t(v), dev_t(lab)), value)
    assert torch.equal(lik.predict_mean_variance(dev_t(mu), dev_t(v))[0], _ops.lik_robustmax_probs(dev_t(mu), dev_t(v), EPS, x, w))


# ---- SVGP -------------------------------------------------------------------------------------------------------------------------
def make_model(case, batch_size=None):
    inp = mo.model_inputs(case)
    lik = likelihoods.MultiClass(case["C"], EPS)
    lik.num_gauss_hermite_points = case["H"]
    np.random.seed(0)
    m = SVGP(inp["x"], inp["y"], kernels.Rbf(case["d"], variance=case["variance"], length_scales=case["length_scale"]),
             inducing_points=inp["z"].copy(), likelihood=lik, batch_size=batch_size)
    m.induced_output_mean.data = torch.tensor(inp["q_mu"])
    m.induced_output_chol_cov.data = so.chol_to_raw(inp["q_sqrt"])
    m.cuda()
    return m, inp


@pytest.mark.parametrize("batch_size", [None, 64], ids=["full", "batch64"])
@pytest.mark.parametrize("case", mo.MODEL_CASES, ids=[c["name"] for c in mo.MODEL_CASES])
def test_model_native_route_equals_torch_route(device, monkeypatch, case, batch_size):
    """loss() and every parameter gradient with NATIVE_EXPECTATION on and off (the same host draw for the minibatch), held to
    tests/_xref.tol of the generator's e64 for this data term (the fp64 oracle's loss is printed beside them)."""
    m, _ = make_model(case, batch_size)
    gold = META["cases"][case["name"]]["full" if batch_size is None else "batch64"]
    calls = []
    real = _ops.lik_expect_robustmax
    monkeypatch.setattr(_ops, "lik_expect_robustmax", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    out = []
    for flag in (True, False):
        monkeypatch.setattr(sparse_gpr, "NATIVE_EXPECTATION", flag)
        m.zero_grad()
        np.random.seed(case["batch_seed"])
        loss = m.loss()
        loss.backward()
        assert len(calls) == 1                                   # on: one call per evaluation; off: none
        out.append((loss.item(), {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters() if p.grad is not None}))
    (got, got_g), (want, want_g) = out
    err = xr.rel_err(got, want)
    print("%s %s: native %.15g torch %.15g oracle %.15g rel err %.2e (tol %.2e)" % (case["name"], batch_size, got, want, gold["loss"], err,
                                                                                   xr.tol(gold["e64_loss"], "loss")))
    assert math.isfinite(want) and err <= xr.tol(gold["e64_loss"], "loss")
    assert set(got_g) == set(want_g) and len(want_g) >= 5
    for n, gw in want_g.items():
        e = xr.rel_err(got_g[n], gw)
        print("   d/d%-32s rel err %.2e" % (n, e))
        assert e <= xr.tol(gold["e64_grad"], "grad"), (n, e)


@pytest.mark.parametrize("case", mo.MODEL_CASES, ids=[c["name"] for c in mo.MODEL_CASES])
def test_predict_y_equals_the_oracle(device, case):
    m, inp = make_model(case)
    gold = GOLD["%s__probs" % case["name"]]
    p, var = m.predict_y(inp["xs"])
    mean_f, var_f = m.predict_f(inp["xs"])
    assert p.shape == (16, case["C"]) and var.shape == p.shape and mean_f.shape == p.shape and var_f.shape == p.shape
    err = xr.abs_err(p, gold)
    print("%s predict_y: abs err %.2e (tol %.2e)" % (case["name"], err, xr.tol(META["cases"][case["name"]]["e64_mean"], "mean")))
    assert err <= xr.tol(META["cases"][case["name"]]["e64_mean"], "mean")
    assert np.array_equal(var, p * (1.0 - p))
    with pytest.raises(NotImplementedError):
        m.predict_y(inp["xs"], diag=False)
    with pytest.raises(NotImplementedError):
        m.predict_y_samples(inp["xs"], n_samples=2)


def test_ten_adam_steps_lower_the_loss(device):
    """the model as constructed (k-means inducing points, the one-hot regression of _init_posterior), full batch."""
    case = mo.MODEL_CASES[0]
    inp = mo.model_inputs(case)
    np.random.seed(3)
    m = SVGP(inp["x"], inp["y"], kernels.Rbf(2), num_inducing_points=20, likelihood=likelihoods.MultiClass(3))
    assert m.induced_output_mean.shape == (20, 3)
    m.cuda()
    first = m.loss(x=m.X, y=m.Y).item()
    with quiet():
        m.optimize(method="Adam", max_iter=10, learning_rate=0.05, verbose=False)
    last = m.loss(x=m.X, y=m.Y).item()
    print("full-batch loss %.4f -> %.4f" % (first, last))
    assert math.isfinite(first) and last < first


def test_blobs_are_separated_after_200_steps(device):
    """three well-separated blobs from q_mu = 0, S_L = I: the training accuracy after 200 Adam steps is 1.0 (the generator
    asserts the same of the torch route on the CPU)."""
    inp, b = mo.blob_inputs(), mo.BLOBS
    lik = likelihoods.MultiClass(b["C"], EPS)
    lik.num_gauss_hermite_points = b["H"]
    np.random.seed(0)
    m = SVGP(inp["x"], inp["y"], kernels.Rbf(2, variance=1.0, length_scales=1.0), inducing_points=inp["z"].copy(), likelihood=lik)
    m.induced_output_mean.data = torch.zeros(b["m"], b["C"], dtype=torch.float64)
    m.induced_output_chol_cov.data = so.chol_to_raw(np.eye(b["m"]))
    m.cuda()
    with quiet():
        losses, _ = m.optimize(method="Adam", max_iter=b["steps"], learning_rate=b["learning_rate"], verbose=False)
    p, _ = m.predict_y(inp["x"])
    acc = float(np.mean(np.argmax(p, 1) == inp["y"][:, 0]))
    print("blobs: loss %.4f -> %.4f (CPU torch route: %.4f -> %.4f), accuracy %.3f" % (losses[0], losses[-1], META["blobs"]["first_loss"],
                                                                                      META["blobs"]["last_loss"], acc))
    assert META["blobs"]["accuracy"] == 1.0 and acc == 1.0
    assert losses[0] == pytest.approx(META["blobs"]["first_loss"], rel=1e-9)


def test_optimize_with_capture_replays_or_falls_back(device):
    case = mo.MODEL_CASES[0]
    m, _ = make_model(case)
    with quiet():
        losses, _ = m.optimize(method="Adam", max_iter=4, verbose=False, capture=True)
    assert losses.shape == (4,) and np.all(np.isfinite(losses))


def test_the_example_runs(device):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "classify_multiclass.py"), "300", "40"], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert "training accuracy" in out.stdout
