"""FITC on the GPU: every case through model.cuda() and the C ABI (csrc/fitc.hip + the streamed pipeline it shares with VFE),
against the goldens of tests/golden/make_fitc_golden.py -- the DENSE N x N evaluation of the same marginal likelihood, in long
double for the loss and the predictions and by fp64 autograd for the gradients.

Tolerances are tests/_xref.tol: max(16 e64, FLOOR[what]) with e64 the distance of the oracle's plain-fp64 dense evaluation from
its long-double one for that case (stored by the maker; never measured against the code under test).  Loss and gradients are
relative to max(1, |reference|) (xr.rel_err), predictions absolute."""
import contextlib
import io

import numpy as np
import pytest
import torch

from gptorch_amd import kernels, likelihoods, rng
from gptorch_amd.models import FITC, GPR, VFE, sparse_gpr
from tests import _fitc_oracle as fo
from tests import _xref as xr
from tests._util import load_json

pytestmark = pytest.mark.gpu

CASES = load_json("fitc_cases.json")
BY_NAME = {c["name"]: c for c in CASES["cases"]}
BIG = BY_NAME["matern32_1000x200x3"]
WIDE = load_json("fitc_wide_case.json")["cases"][0]                          # M = 1100 (make_fitc_golden.py --wide)


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def cuda_model(case, cls=None):
    inp = fo.case_inputs(case)
    m = fo.build_model(case, inp, cls)
    m.cuda()
    return inp, m


def check_loss_and_grads(case, m):
    m.zero_grad()
    loss = m.loss()
    loss.backward()
    assert loss.dim() == 0 and loss.is_cuda
    err = xr.rel_err(loss.item(), case["loss_ld"])
    print("%s: loss %.12f golden %.12f rel err %.2e (tol %.1e)" % (case["name"], loss.item(), case["loss_ld"], err, xr.tol(case["e64"]["loss"], "loss")))
    assert err <= xr.tol(case["e64"]["loss"], "loss")
    params = dict(m.named_parameters())
    for on, mn in fo.model_names(case).items():
        got = params[mn].grad.detach().cpu().numpy()
        want = np.asarray(case["grads"][on]).reshape(got.shape)
        err = xr.rel_err(got, want)
        print("   d/d%-32s rel err %.2e of max %.2e" % (mn, err, np.max(np.abs(want))))
        assert err <= xr.tol(case["e64"]["grad"], "grad"), mn
    return loss


def check_predictions(case, inp, m):
    xs = torch.tensor(inp["xs"]).cuda()
    e = case["e64"]
    mu, var = m.predict_f(xs)
    mu2, cov = m.predict_f(xs, diag=False)
    errs = (xr.abs_err(mu, case["mean_pred"]), xr.abs_err(var[:, 0], case["var_pred"]), xr.abs_err(cov, case["cov_pred"]))
    print("   predict_f: mean %.2e var %.2e cov %.2e" % errs)
    assert tuple(var.shape) == tuple(mu.shape) and torch.equal(mu, mu2)
    assert errs[0] <= xr.tol(e["mean"], "mean") and errs[1] <= xr.tol(e["var"], "var") and errs[2] <= xr.tol(e["cov"], "var")
    my, vy = m.predict_y(xs)
    assert xr.abs_err(my, case["mean_pred"]) <= xr.tol(e["mean"], "mean")
    assert xr.abs_err(vy[:, 0], np.asarray(case["var_pred"]) + case["noise"]) <= xr.tol(e["var"], "var")
    mean_n, var_n = m.predict_y(inp["xs"])                                   # the public route: numpy in -> numpy out
    assert isinstance(mean_n, np.ndarray) and xr.abs_err(var_n[:, 0], np.asarray(case["var_pred"]) + case["noise"]) <= xr.tol(e["var"], "var")


@pytest.mark.parametrize("case", CASES["cases"], ids=[c["name"] for c in CASES["cases"]])
def test_golden_cases(device, case):
    """log_likelihood, every gradient (Z and the mean included), predict_f (diag and full covariance) and predict_y."""
    inp, m = cuda_model(case)
    assert m.X.shape[0] <= sparse_gpr.CHUNK_ROWS                             # one chunk
    check_loss_and_grads(case, m)
    check_predictions(case, inp, m)
    assert m._state_for_predict(m.X) is m._state_for_predict(m.X)            # the state is kept between predictions


def test_wide_golden_case(device):
    """M = 1100 > 1024 (N = 1400, dy = 2, Z = the first 1100 rows of X: lambda = noise on those rows): the <32> instantiation of
    the forward row kernel and 18 column tiles of the backward rows, against the dense N x N oracle like every golden case."""
    assert WIDE["m"] > 1024 and WIDE["name"] == "matern32_1400x1100x2"
    inp, m = cuda_model(WIDE)
    check_loss_and_grads(WIDE, m)
    check_predictions(WIDE, inp, m)


def test_blocked_right_solve_matches_the_leaf_chain(device, monkeypatch):
    """FITC's backward recomputes A_c^T through sparse_gpr._solve_chunk and must get the forward's bits, whichever right-solve that
    is.  N = 4608, M = 1100 (the second 1024-block of L_uu is ragged), chunks of 2048 rows (two and a tail of 512): with the
    blocked solve switched on (BLOCKED_SOLVE_MIN_M = 1024) the same likelihood and gradients as down the leaf chain -- the
    tolerances of test_vfe_blocked_right_solve_matches_the_leaf_chain --, and the likelihood against the oracle's M-sized fp64
    evaluation (1e-9 relative, as that test holds the VFE bound to its oracle)."""
    n, mq, d = 4608, 1100, 3
    x, y = rng.make_regression(n, d, 1, seed=41)
    z = rng.normal(42, (mq, d)) * 2.0
    res = {}
    for name, thr in (("blocked", 1024), ("chain", 10 ** 9)):
        monkeypatch.setattr(sparse_gpr, "BLOCKED_SOLVE_MIN_M", thr)
        monkeypatch.setattr(sparse_gpr, "CHUNK_ROWS", 2048)
        assert sparse_gpr._blocked_solve(mq, n) == (name == "blocked")
        assert [r for _, r in sparse_gpr._chunks(n, sparse_gpr._chunk_rows(n))] == [2048, 2048, 512]
        mod = FITC(x, y, kernels.Matern52(d, variance=1.2, length_scales=0.6), inducing_points=z.copy(), likelihood=likelihoods.Gaussian(variance=0.1))
        mod.cuda()
        loss = mod.loss()
        loss.backward()
        res[name] = (loss.item(), {k: p.grad.clone() for k, p in mod.named_parameters() if p.grad is not None})
    (lb, gb), (lc, gc) = res["blocked"], res["chain"]
    print("fitc blocked %.12f chain %.12f rel diff %.2e" % (lb, lc, abs(lb - lc) / abs(lc)))
    assert abs(lb - lc) < 1e-10 * abs(lc), (lb, lc)
    assert set(gb) == set(gc) and len(gc) >= 4
    for k in gc:
        diff = (gb[k] - gc[k]).abs().max().item()
        print("   d/d%-28s max diff %.2e of max %.2e" % (k, diff, gc[k].abs().max().item()))
        assert diff < 1e-7 * max(1.0, gc[k].abs().max().item()), k
    o = fo.FITCOracle(x, y, z, dict(kind="Matern52", variance=1.2, length_scales=0.6), 0.1)
    with torch.no_grad():
        ref = o.woodbury_lml(*o._inputs()).item()
    print("   oracle (Woodbury, fp64) %.12f rel diff %.2e" % (ref, abs(-lb - ref) / abs(ref)))
    assert abs(-lb - ref) < 1e-9 * abs(ref), (lb, ref)


@pytest.mark.parametrize("chunk", [None, 256], ids=["single_chunk", "multi_chunk"])
def test_multi_chunk(device, monkeypatch, chunk):
    """N = 1000 in chunks of 256 rows: three whole chunks and a ragged tail of 232 rows over both lanes -- the same likelihood."""
    if chunk is not None:
        monkeypatch.setattr(sparse_gpr, "CHUNK_ROWS", chunk)
    inp, m = cuda_model(BIG)
    n, nc = m.X.shape[0], sparse_gpr._chunk_rows(m.X.shape[0])
    sizes = [r for _, r in sparse_gpr._chunks(n, nc)]
    assert sizes == ([1000] if chunk is None else [256, 256, 256, 232]) and sparse_gpr.LANES == 2
    check_loss_and_grads(BIG, m)
    check_predictions(BIG, inp, m)


def test_bitwise_determinism(device, monkeypatch):
    """two evaluations at the multi-chunk setting -> bitwise-equal loss and gradients (fixed summation orders, no atomics)."""
    monkeypatch.setattr(sparse_gpr, "CHUNK_ROWS", 256)
    _, m = cuda_model(BIG)
    assert sparse_gpr._chunk_rows(m.X.shape[0]) == 256
    runs = []
    for _ in range(2):
        m.zero_grad()
        loss = m.loss()
        loss.backward()
        runs.append([loss.detach().clone()] + [p.grad.detach().clone() for p in m.parameters() if p.grad is not None])
    assert len(runs[0]) == 5
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_collapses_to_the_exact_gp_when_z_is_x(device):
    """Z = X (N = M = 40, dy = 9): Lambda = s2 I and Q = K, so FITC's likelihood is GPR's."""
    case = BY_NAME["matern52_ard_130x40x9"]
    inp = fo.case_inputs(case)
    x, y = inp["x"][:case["m"]].copy(), inp["y"][:case["m"]].copy()
    fitc = FITC(x, y, fo.build_kernel(kernels, case), inducing_points=x.copy(), likelihood=likelihoods.Gaussian(variance=case["noise"]))
    gpr = GPR(x, y, fo.build_kernel(kernels, case), likelihood=likelihoods.Gaussian(variance=case["noise"]))
    fitc.cuda(), gpr.cuda()
    a, b = fitc.log_likelihood().item(), gpr.log_likelihood().item()
    print("Z = X: FITC %.12f GPR %.12f rel err %.2e" % (a, b, xr.rel_err(a, b)))
    assert xr.rel_err(a, b) <= xr.tol(0.0, "loss")


@pytest.mark.parametrize("case", [c for c in CASES["cases"] if c.get("mean") is None], ids=[c["name"] for c in CASES["cases"] if c.get("mean") is None])
def test_is_not_the_vfe_bound(device, case):
    _, fitc = cuda_model(case)
    _, vfe = cuda_model(case, VFE)
    a, b = fitc.log_likelihood().item(), vfe.log_likelihood().item()
    print("%s: FITC %.8f VFE %.8f" % (case["name"], a, b))
    assert abs(a - b) > 1e-6


def test_adam_steps_follow_the_oracle(device):
    """optimize(method="Adam", max_iter=5) lowers the loss along the trajectory of torch's CPU Adam on the dense oracle."""
    t = CASES["trajectory"]
    _, m = cuda_model(t)
    with quiet():
        losses, _ = m.optimize(method="Adam", max_iter=t["steps"], learning_rate=t["learning_rate"], verbose=False)
    want = np.asarray(t["losses"])
    err = np.max(np.abs(losses - want) / np.maximum(1.0, np.abs(want)))
    print("fitc adam trajectory: losses %s max rel err %.2e" % (losses, err))
    assert losses[-1] < losses[0] and all(a > b for a, b in zip(losses, losses[1:]))
    assert err < 1e-7


def test_million_rows_in_chunk_sized_memory(device):
    """one loss(); backward() at N = 2^20, M = 256, d = 4, dy = 1: the peak allocation (absolute) stays below ONE [N, M] fp64
    array (a single held Kuf, 2.1 GB), and everything is finite."""
    n, d, mq = 1 << 20, 4, 256
    g = torch.Generator(device="cuda").manual_seed(23)
    x = torch.randn(n, d, dtype=torch.float64, device="cuda", generator=g)
    y = torch.sin(x.sum(1, keepdim=True)) + 0.1 * torch.randn(n, 1, dtype=torch.float64, device="cuda", generator=g)
    z = x[:mq].cpu().numpy() + 0.01
    m = FITC(x[:2000].cpu().numpy(), y[:2000].cpu().numpy(), kernels.Matern52(d, length_scales=1.5), inducing_points=z,
             likelihood=likelihoods.Gaussian(variance=0.05))
    m.cuda()
    m.X, m.Y = x, y
    assert m.num_data == n
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = m.loss()
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print("N = 2^20, M = 256: loss %.6f, peak %.2f GB (growth %.2f GB) of a %.2f GB Kuf" % (loss.item(), peak / 1e9, (peak - base) / 1e9, n * mq * 8 / 1e9))
    assert peak < n * mq * 8                                                 # everything alive, data and model included
    assert bool(torch.isfinite(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.requires_grad)
