"""SVGP on the GPU: every case through model.cuda() and the C ABI (csrc/svgp.hip + the shared M-sized algebra), against the
reference's known answers, the goldens of tests/golden/make_svgp_golden.py and the host oracle tests/_svgp_oracle.py.
Tolerances are the sibling model's: bound 1e-8 relative and predictions 1e-8 (test_vfe_medium_golden), 1e-8 ABSOLUTE on the
well-conditioned bound (test_vfe_wellconditioned_golden_absolute), gradients 1e-7 x max|reference gradient| per block
(tests/test_gpu_parity.py), trajectory as test_adam_trajectory_golden."""
import contextlib
import io
import math

import numpy as np
import pytest
import torch

import gptorch_amd
from gptorch_amd import kernels, likelihoods, mean_functions, param, rng, settings
from gptorch_amd.models import SVGP, sparse_gpr
from tests import _svgp_oracle as so
from tests._util import load_npz
from tests.test_svgp_host import CASES, golden_grad, inputs_of

pytestmark = pytest.mark.gpu


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def reference_model(device, batch_size=None):
    """test/test_models/test_sparse_gpr.py:314-336."""
    f, g = load_npz("ref_sparse_gpr_fixtures.npz"), load_npz("ref_svgp_fixtures.npz")
    kern = kernels.Matern32(1)
    kern.length_scales.data = torch.zeros(1, dtype=torch.float64)
    kern.variance.data = torch.zeros(1, dtype=torch.float64)
    m = SVGP(f["x"], f["y"], kern, inducing_points=f["z"], likelihood=likelihoods.Gaussian(variance=1.0),
             mean_function=mean_functions.Zero(1), batch_size=batch_size)
    m.induced_output_mean.data = torch.tensor(g["q_mu"])
    m.induced_output_chol_cov.data = m.induced_output_chol_cov._transform.inv(torch.tensor(g["l_s"]))
    m.cuda()
    return m, f, g


def test_reference_known_answers(device):
    """test_compute_loss / test_predict / *_cuda of the reference's TestSVGP."""
    m, f, g = reference_model(device)
    loss = m.loss()
    assert isinstance(loss, torch.Tensor) and loss.dim() == 0 and loss.is_cuda
    print("svgp known answer: %.15f (reference run %.15f)" % (loss.item(), g["svgp_loss_reference_run"][0]))
    assert loss.item() == pytest.approx(9.534628739243518)
    assert abs(loss.item() - g["svgp_loss_reference_run"][0]) < 1e-9
    loss_xy = m.loss(x=m.X, y=m.Y)
    assert loss_xy.item() == loss.item()
    with pytest.raises(ValueError):
        m.loss(x=m.X[: m.X.shape[0] // 2], y=m.Y)
    mb = SVGP(f["x"], f["y"], m.kernel, batch_size=1)
    mb.cuda()
    loss_mb = mb.loss()
    assert loss_mb.dim() == 0 and loss_mb.is_cuda
    full_mb, _, _ = reference_model(device, batch_size=f["x"].shape[0])
    assert full_mb.loss().item() == pytest.approx(loss.item(), rel=1e-12)
    xs = torch.tensor(f["x_test"]).cuda()
    mu, cov = m._predict(xs, diag=False)
    assert mu.is_cuda and cov.is_cuda
    assert np.max(np.abs(mu.cpu().numpy().ravel() - g["svgp_y_mean"].ravel())) < 1e-8
    assert np.max(np.abs(cov.cpu().numpy() - g["svgp_y_cov"])) < 1e-8
    mu_d, var_d = m._predict(xs)
    assert tuple(var_d.shape) == tuple(mu_d.shape)
    assert np.max(np.abs(var_d.cpu().numpy()[:, 0] - np.diag(g["svgp_y_cov"]))) < 1e-8
    # the public route: numpy in -> numpy out
    mu_n, var_n = m.predict_y(f["x_test"])
    assert np.max(np.abs(var_n[:, 0] - np.diag(g["svgp_y_cov"]) - 1.0)) < 1e-8


def check_grads(model, want_of, tol=1e-7):
    for name, p in model.named_parameters():
        if name not in want_of:
            continue
        want = want_of[name]
        got = p.grad.detach().cpu().numpy()
        scale = float(np.max(np.abs(want)))
        err = float(np.max(np.abs(got - want.reshape(got.shape))))
        print("   d/d%-32s err %.2e of max %.2e" % (name, err, scale))
        assert err < tol * scale, (name, err, scale)


@pytest.mark.parametrize("case", CASES["cases"], ids=[c["name"] for c in CASES["cases"]])
def test_golden_cases(device, case):
    arrays = load_npz("svgp_cases.npz")
    inp = inputs_of(case, arrays)
    m = so.build_model(gptorch_amd, case, inp)
    m.cuda()
    idx = None if inp["idx"] is None else torch.as_tensor(inp["idx"], device=m.X.device)
    for ev in case["evals"]:
        m.zero_grad()
        loss = m.loss() if ev["tag"] == "full" else m.loss(x=m.X[idx], y=m.Y[idx])
        loss.backward()
        err = abs(loss.item() - ev["loss"])
        print("%s/%s: loss %.10f golden %.10f |diff| %.2e" % (case["name"], ev["tag"], loss.item(), ev["loss"], err))
        assert err < 1e-8 * abs(ev["loss"])
        if case.get("absolute"):
            assert err < 1e-8                        # cond K(Z) = case["cond_Kuu"]: no ladder rung, 1e-8 ABSOLUTE
        shapes = {n: tuple(p.shape) for n, p in m.named_parameters()}
        check_grads(m, {n: golden_grad(g, arrays, shapes[n]) for n, g in ev["grads"].items()})
    xs = torch.tensor(inp["xs"]).cuda()
    mu, var = m._predict(xs)
    _, cov = m._predict(xs, diag=False)
    assert np.max(np.abs(mu.cpu().numpy() - np.asarray(case["mean_pred"]))) < 1e-8
    assert np.max(np.abs(var.cpu().numpy()[:, 0] - np.asarray(case["var_pred"]))) < 1e-8
    assert np.max(np.abs(cov.cpu().numpy() - np.asarray(case["cov_pred"]))) < 1e-8


def test_adam_trajectory_golden(device):
    """20 minibatch Adam steps under the reference's np.random.seed: the host draw is the reference's."""
    t = CASES["trajectory"]
    arrays = load_npz("svgp_cases.npz")
    inp = so.case_inputs(t)
    m = so.build_model(gptorch_amd, t, inp, batch_size=t["batch_size"])
    m.cuda()
    np.random.seed(t["np_seed"])
    with quiet():
        losses, _ = m.optimize(method="Adam", max_iter=t["steps"], learning_rate=t["learning_rate"], verbose=False)
    want = np.asarray(t["losses"])
    err = np.max(np.abs(losses - want) / np.maximum(1.0, np.abs(want)))
    print("svgp adam trajectory: max rel loss err %.2e" % err)
    assert err < 1e-8
    for name, p in m.named_parameters():
        w = golden_grad("npz:trajectory.final." + name, arrays, tuple(p.shape))
        assert np.max(np.abs(p.detach().cpu().numpy() - w)) < 1e-8, name
    assert not m._can_capture("Adam")


def _ragged_model(n, m_, dy, d=3, kind="Matern52", seed=11):
    case = dict(n=n, d=d, dy=dy, m=m_, kernel=dict(kind=kind, variance=1.2, length_scales=1.3), noise=0.15, seed_x=seed, seed_z=seed + 1,
                seed_q=seed + 2, seed_xs=seed + 3)
    inp = so.case_inputs(case)
    model = so.build_model(gptorch_amd, case, inp)
    model.cuda()
    return case, inp, model


@pytest.mark.parametrize("shape", [(1000, 200, 3), (37, 5, 1), (130, 40, 9), (1300, 1100, 5, 6, "Matern32")],
                         ids=["1000x200x3", "37x5x1", "130x40x9", "1300x1100x5"])
def test_ragged_shapes_against_the_host_oracle(device, shape):
    """nb, M, dy not multiples of 16: padded lanes contribute exact zeros (dy = 9: more output columns than one pass of either
    row kernel takes; M = 1100: the second SV_JT tile of the marginals and 18 column tiles of the backward rows, d = 6 with
    Matern32 -- cond K(Z) = 4e3 on the host, where the oracle's loss moves by 1e-16 under a 1-ulp perturbation of Z)."""
    case, inp, m = _ragged_model(*shape)
    o = so.oracle_for(case, inp)
    want, grads = o.loss_and_grads()
    loss = m.loss()
    loss.backward()
    print("ragged %s: loss %.10f oracle %.10f" % (shape, loss.item(), want))
    assert abs(loss.item() - want) < 1e-8 * abs(want)
    check_grads(m, {mn: grads[on] for on, mn in so.model_names(case).items()})
    mu, var = m._predict(torch.tensor(inp["xs"]).cuda())
    omu, ovar = o.predict_f(inp["xs"])
    assert np.max(np.abs(mu.cpu().numpy() - omu)) < 1e-8 and np.max(np.abs(var.cpu().numpy()[:, 0] - ovar)) < 1e-8


@pytest.mark.parametrize("chunk", [None, 256], ids=["single_chunk", "multi_chunk"])
def test_bitwise_determinism(device, monkeypatch, chunk):
    """the same explicit batch twice -> bitwise-equal loss and gradients (fixed summation orders, no atomics)."""
    if chunk is not None:
        monkeypatch.setattr(sparse_gpr, "CHUNK_ROWS", chunk)                 # 1000 rows -> 3 whole chunks and a ragged tail
    case, inp, m = _ragged_model(1000, 200, 3)
    runs = []
    for _ in range(2):
        m.zero_grad()
        loss = m.loss(x=m.X, y=m.Y)
        loss.backward()
        runs.append([loss.detach().clone()] + [p.grad.detach().clone() for p in m.parameters() if p.grad is not None])
    assert len(runs[0]) >= 6
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    if chunk is not None:                                                    # and the chunked evaluation is the same bound
        o = so.oracle_for(case, inp)
        want, grads = o.loss_and_grads()
        assert abs(runs[0][0].item() - want) < 1e-8 * abs(want)
        check_grads(m, {mn: grads[on] for on, mn in so.model_names(case).items()})


def test_gaussian_shortcut_equals_generic_route(device, monkeypatch):
    """value and gradients of the Gaussian data term with and without the sqrt / square round trip of propagate_log: 1e-12."""
    case, inp, m = _ragged_model(500, 48, 2)
    out = []
    for flag in (True, False):
        monkeypatch.setattr(sparse_gpr, "GAUSSIAN_SHORTCUT", flag)
        m.zero_grad()
        loss = m.loss()
        loss.backward()
        out.append((loss.item(), {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters() if p.grad is not None}))
    assert abs(out[0][0] - out[1][0]) < 1e-12 * abs(out[1][0])
    for n, g in out[1][1].items():
        assert np.max(np.abs(out[0][1][n] - g)) < 1e-12 * np.max(np.abs(g)), n


class ScaledGaussian(likelihoods.Likelihood):
    """a user likelihood with its own closed-form propagate_log (sparse_gpr.py:276-283's extension point): Gaussian noise
    whose variance is `scale` times a trainable parameter."""

    def __init__(self, scale=2.0):
        super().__init__()
        self.scale = scale
        self.variance = param.Param(torch.tensor([0.2], dtype=torch.float64),
                                                transform=settings.DefaultPositiveTransform())

    def propagate_log(self, qf, targets):
        s2 = self.scale * self.variance.transform()
        return -0.5 * (targets.nelement() * (math.log(2.0 * math.pi) + torch.log(s2))
                       + (torch.sum((targets - qf.loc) ** 2) + qf.variance.sum()) / s2)


def test_custom_likelihood_trains(device):
    x, y = rng.make_regression(400, 2, 1, seed=5)
    np.random.seed(3)
    m = SVGP(x, y, kernels.Rbf(2), num_inducing_points=20, likelihood=ScaledGaussian())
    m.cuda()
    with quiet():
        losses, _ = m.optimize(method="Adam", max_iter=3, verbose=False)      # full batch, the default learning rate (0.01)
    print("custom likelihood losses", losses)
    assert losses[0] > losses[1] > losses[2]


def test_million_rows_in_chunk_sized_memory(device):
    """full-batch bound + backward at N = 2^20, d = 8, dy = 1, M = 1024: the growth of the peak allocation stays below ONE
    [N, M] fp64 array (8.6 GB), and the value equals the mean of 16 explicit 65536-row pieces (each piece rescales its data
    term by N / 65536 and carries the KL once, so their mean is the bound), 1e-10 relative."""
    n, d, mq = 1 << 20, 8, 1024
    g = torch.Generator(device="cuda").manual_seed(17)
    x = torch.randn(n, d, dtype=torch.float64, device="cuda", generator=g)
    y = torch.sin(x.sum(1, keepdim=True)) + 0.1 * torch.randn(n, 1, dtype=torch.float64, device="cuda", generator=g)
    z = x[:mq].cpu().numpy() + 0.01
    np.random.seed(0)
    m = SVGP(x[:2000].cpu().numpy(), y[:2000].cpu().numpy(), kernels.Matern52(d, length_scales=2.0), inducing_points=z)
    m.cuda()
    m.X, m.Y = x, y
    assert m.num_data == n
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = m.loss()
    loss.backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    print("N = 2^20, M = 1024: loss %.6f, peak growth %.2f GB" % (loss.item(), growth / 1e9))
    assert growth < n * mq * 8
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.requires_grad)
    with torch.no_grad():
        pieces = torch.stack([m.loss(x=x[c:c + 65536], y=y[c:c + 65536]) for c in range(0, n, 65536)])
    want = pieces.mean().item()
    assert abs(loss.item() - want) < 1e-10 * abs(want), (loss.item(), want)
