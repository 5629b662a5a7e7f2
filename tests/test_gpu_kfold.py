"""The k-fold objective of GPR on the GPU: the entry points of csrc/kfold.hip at their tile edges (bitwise for the two gathers),
the folds' terms against the long-double oracle, every golden case of tests/golden/make_kfold_golden.py through model.cuda(), the
dense route, the NaN rule, determinism, fitting, and the guards that keep the feature out of everything that existed before it.

Tolerances.  tests/_xref.tol = max(16 e64, FLOOR[what]) with e64 the distance of the oracle's plain-fp64 statement from its
long-double one (stored by the maker, or measured here between the two host statements; never against the code under test); loss,
gradients, log-determinants and quadratic forms relative to max(1, |reference|) (xr.rel_err), predictions and q absolute.  The
value of gpn_kfold_terms additionally gets the rounding of its fixed-order sum (test_terms).  The gathers are copies: bitwise."""
import contextlib
import io
import json

import numpy as np
import pytest
import torch

from gptorch_amd import _native, _ops, kernels, likelihoods, mean_functions, rng
from gptorch_amd.models import GPR, batched_loss_and_grad, multi_start_optimize
from tests import _kfold_oracle as ko
from tests import _xref as xr
from tests._util import load_npz
from tests.golden import make_kfold_golden as maker

pytestmark = pytest.mark.gpu

GOLD = load_npz("kfold_cases.npz")
CASES = {c["name"]: c for c in json.loads(str(GOLD["meta"]))["cases"]}
U = 2.0 ** -53
LD = ko.LD
SENTINEL = -7.25
GUARD = 512                                   # doubles of canary before and after every buffer under test (even: keeps 16-byte alignment)


def shuffled(n, sizes, seed):
    order = np.argsort(rng.uniform(seed, n), kind="stable")
    return [np.asarray(p, dtype=np.int64) for p in np.split(order, np.cumsum(sizes)[:-1])]


# the partitions of the issue's table: (n, folds) -- an int k, or index arrays (contiguous or shuffled: unsorted lists)
PARTITIONS = {
    "7_k2": (7, 2),
    "64_32_32": (64, [np.arange(32), np.arange(32, 64)]),
    "64_63_1": (64, [np.arange(63), np.arange(63, 64)]),
    "65_k4": (65, 4),
    "203_shuffled": (203, shuffled(203, [64, 65, 48, 26], 339)),
    "203_k6": (203, 6),
    "300_shuffled": (300, shuffled(300, [129, 128, 43], 353)),
}
DY_OF = {"7_k2": 1, "64_32_32": 2, "64_63_1": 5, "65_k4": 1, "203_shuffled": 5, "203_k6": 2, "300_shuffled": 1}


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def cuda(a):
    return torch.tensor(np.asarray(a, dtype=np.float64)).cuda()


def spd(n, seed):
    """a random SPD matrix standing in for P, diagonally dominant enough to be well scaled."""
    g = rng.normal(seed, (n, n + 3))
    return g @ g.T / (n + 3) + 0.5 * np.eye(n)


def lower_buffer(M, ld, device, odd=False):
    """the lower triangle of M in a [round_up(n, 64), ld] buffer, NaN everywhere else: nothing else may be read.  odd: an odd leading
    dimension and a base that is 8-byte but not 16-byte aligned (tests/test_gpu_loo.py test_loo_scale's odd_ld, and one element on)."""
    n = M.shape[0]
    rows = _ops.round_up(n, 64)
    if odd:
        ld += 1 - ld % 2
        flat = torch.full((rows * ld + 2,), float("nan"), dtype=torch.float64, device=device)
        off = 1 if flat.data_ptr() % 16 == 0 else 0
        buf = flat[off:off + rows * ld].view(rows, ld)
        assert buf.data_ptr() % 16 == 8 and ld % 2 == 1
    else:
        buf = torch.full((rows, ld), float("nan"), dtype=torch.float64, device=device)
    buf[:n, :n] = cuda(np.tril(M) + np.triu(np.full((n, n), np.nan), 1))
    return buf


def guarded(numel, device):
    """a buffer of `numel` doubles with a canary on both sides, all of it filled with the canary: (whole, the buffer's view)"""
    whole = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=device)
    return whole, whole[GUARD:GUARD + numel]


# ---- the two gathers: pure copies -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odd_ld", [False, True], ids=["factor_ld", "odd_ld"])
@pytest.mark.parametrize("part", list(PARTITIONS))
def test_fold_gather(device, part, odd_ld):
    """P[I, I] (entry (i, j) = P[max, min] of the lower triangle), the identity padding and a_I^T in the extra rows, bitwise equal to
    numpy indexing of the symmetrised P; a canary fill shows that nothing outside rows [0, m_max + dy) x columns [0, m_max) of a
    fold's buffer is written (so a zeroed factor buffer keeps its zero padding)."""
    n, folds = PARTITIONS[part]
    dy = DY_OF[part]
    lib = _native.lib()
    table = _ops.FoldTable(folds, n, device)
    k, m = table.k, table.m_max
    P = spd(n, 300 + n)
    Psym = np.tril(P) + np.tril(P, -1).T
    a = rng.normal(400 + n, (n, dy))
    Kinv = lower_buffer(P, int(lib.gpn_factor_ld(n, dy)), device, odd=odd_ld)
    at = cuda(a.T).contiguous()                # (torch.tensor keeps the transposed view's strides; the entry point takes rows of n)
    ld, rows = int(lib.gpn_factor_ld(m, dy)), int(lib.gpn_factor_rows(m, dy))
    whole, A = guarded(k * rows * ld, device)
    off, idx = table.on(device)
    st = lib.gpn_kfold_gather(_ops._stream(device), n, dy, _ops._ptr(Kinv), Kinv.stride(0), _ops._ptr(at), n, k, _ops._ptr(off), _ops._ptr(idx), m,
                              _ops._ptr(A), ld, rows * ld)
    assert st == 0
    want = np.full((k, rows, ld), SENTINEL)
    for f, I in enumerate(table.parts):
        mf = I.size
        want[f, :m, :m] = np.eye(m)
        want[f, :mf, :mf] = Psym[np.ix_(I, I)]
        want[f, m:m + dy, :m] = 0.0
        want[f, m:m + dy, :mf] = a[I].T
    assert np.array_equal(A.view(k, rows, ld).cpu().numpy(), want)
    assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + k * rows * ld:] == SENTINEL).all())


@pytest.mark.parametrize("odd_ld", [False, True], ids=["factor_ld", "odd_ld"])
@pytest.mark.parametrize("part", list(PARTITIONS))
def test_column_gather(device, part, odd_ld):
    """P[:, I_f] as FULL columns (rows above the diagonal from the mirror) into [k, round_up(n, 16), round_up(m_max, 16)], bitwise,
    zero padded; the canary around the buffer is untouched."""
    n, folds = PARTITIONS[part]
    lib = _native.lib()
    table = _ops.FoldTable(folds, n, device)
    k, m = table.k, table.m_max
    P = spd(n, 500 + n)
    Psym = np.tril(P) + np.tril(P, -1).T
    Kinv = lower_buffer(P, int(lib.gpn_factor_ld(n, 1)), device, odd=odd_ld)
    npad, mpad = _ops.round_up(n, 16), _ops.round_up(m, 16)
    assert lib.gpn_kfold_columns_work_bytes(n, k, m) == 8 * k * npad * mpad
    whole, C = guarded(k * npad * mpad, device)
    assert C.data_ptr() % 16 == 0
    off, idx = table.on(device)
    st = lib.gpn_kfold_columns(_ops._stream(device), n, _ops._ptr(Kinv), Kinv.stride(0), k, _ops._ptr(off), _ops._ptr(idx), m, _ops._ptr(C), mpad,
                               npad * mpad)
    assert st == 0
    want = np.zeros((k, npad, mpad))
    for f, I in enumerate(table.parts):
        want[f, :n, :I.size] = Psym[:, I]
    assert np.array_equal(C.view(k, npad, mpad).cpu().numpy(), want)
    assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + k * npad * mpad:] == SENTINEL).all())
    # the wrapper's own buffer: the same bits
    assert np.array_equal(_ops.kfold_columns(Kinv, n, table).cpu().numpy(), want)


# ---- weights, terms, value --------------------------------------------------------------------------------------------------------------
def run_terms(P, a, table, device):
    """the forward's fold steps from a given fp64 P (lower triangle uploaded) and a: gather, the lock-step factorisation, the terms"""
    n, dy = a.shape
    Kinv = lower_buffer(P, int(_native.lib().gpn_factor_ld(n, dy)), device)
    fb = _ops.FactorBatch(table.k, table.m_max, dy, device)
    _ops.kfold_gather(Kinv, cuda(a.T), n, dy, table, fb)
    out3, Uf = _ops.kfold_factorise(fb)
    qt, var, Wt, value = _ops.kfold_terms(table, n, dy, fb, Uf, out3=out3, info=fb.info)
    return fb, out3, Uf, qt, var, Wt, value


def host_P_a(n, dy, seed):
    """an fp64 P = Kyy^-1 of an Rbf model and a = P r, computed on the host"""
    x, y = rng.make_regression(n, 2, dy, seed=seed)
    K = np.asarray(xr.K("Rbf", x, None, 1.3, 0.8), dtype=np.float64) + 0.05 * np.eye(n)
    P = np.linalg.inv(K)
    P = 0.5 * (P + P.T)
    return P, P @ y


@pytest.mark.parametrize("part", list(PARTITIONS))
def test_terms(device, part):
    """per-fold log|P_f| and a_I^T q_I, q and the held-out variances in data order, and the value, from an fp64 P and a computed on
    the host, against the long-double evaluation of the same P and a (ko.kfold_terms); e64 = the fp64 numpy evaluation's distance.
    Value: its own tolerance, plus the rounding of the fixed-order sum -- per fold dy * s0 - s1 / 2 (3 roundings), 6 shuffle levels
    + 2 for the four wavefronts + ceil(k / 256) sequential terms, and two more roundings for the constant -1/2 n dy log 2 pi (its
    own, and its addition), over sum |fold term| + |constant|, as tests/test_gpu_loo.py test_loo_terms derives its allowance."""
    n, folds = PARTITIONS[part]
    dy = DY_OF[part]
    table = _ops.FoldTable(folds, n, device)
    P, a = host_P_a(n, dy, 600 + n)
    q_ld, v_ld, _, ldet_ld, quad_ld, val_ld = ko.kfold_terms(P, a, table.parts, LD)
    q_64, v_64, _, ldet_64, quad_64, val_64 = ko.kfold_terms(P, a, table.parts, np.float64)
    fb, out3, Uf, qt, var, Wt, value = run_terms(P, a, table, device)
    assert fb.info.tolist() == [0] * table.k
    o = out3.cpu().numpy()
    checks = (("logdet", xr.rel_err(2 * o[:, 0], ldet_ld), xr.tol(xr.rel_err(ldet_64, ldet_ld), "loss")),
              ("quad", xr.rel_err(o[:, 1], quad_ld), xr.tol(xr.rel_err(quad_64, quad_ld), "loss")),
              ("q", xr.abs_err(qt.t(), q_ld), xr.tol(xr.abs_err(q_64, q_ld), "mean")),
              ("var", xr.abs_err(var, v_ld), xr.tol(xr.abs_err(v_64, v_ld), "var")))
    for name, err, tol in checks:
        print("terms %s %s: err %.2e tol %.1e" % (part, name, err, tol))
        assert err <= tol, name
    terms = LD(0.5) * (dy * ldet_ld - quad_ld)
    const = 0.5 * n * dy * np.log(2 * np.pi)
    depth = 3 + 6 + 2 + (table.k + 255) // 256 + 2
    tol = xr.tol(xr.rel_err(val_64, val_ld), "loss") * max(1.0, abs(float(val_ld))) + depth * U * float(np.sum(np.abs(terms)) + const)
    print("terms %s value: err %.3e tol %.3e" % (part, abs(float(value.item() - val_ld)), tol))
    assert abs(float(value.item() - val_ld)) <= tol
    # W_f^T: sqrt(dy / 2) U_f^T and sqrt(1/2) q_I^T, one rounding each (the bits of the fp64 product); zero everywhere else
    m, mp, wp = table.m_max, _ops.round_up(table.m_max, 16), _ops.round_up(table.m_max + dy, 16)
    Wt = Wt.view(table.k, wp, mp).cpu().numpy()
    Un = Uf.view(table.k, fb.rows, fb.ld).cpu().numpy()
    qn = qt.cpu().numpy()
    want = np.zeros_like(Wt)
    for f, I in enumerate(table.parts):
        want[f, :I.size, :I.size] = np.sqrt(0.5 * dy) * np.triu(Un[f, :I.size, :I.size]).T
        want[f, m:m + dy, :I.size] = np.sqrt(0.5) * qn[:, I]
    assert np.array_equal(Wt, want)
    # the same call twice gives the same bits
    again = run_terms(P, a, table, device)
    assert all(torch.equal(x, y) for x, y in zip((out3, qt, var, value), (again[1], again[3], again[4], again[6])))


def test_a_fold_block_that_is_not_positive_definite_gives_nan(device):
    """P_f gets no jitter and nothing is clamped: one fold block with a negative diagonal entry makes the value NaN (and its info
    non-zero); the same call on the good P is finite.  Numeric only."""
    n, dy = 203, 2
    table = _ops.FoldTable(PARTITIONS["203_shuffled"][1], n, device)
    P, a = host_P_a(n, dy, 700)
    good = run_terms(P, a, table, device)
    assert good[0].info.tolist() == [0] * 4 and bool(torch.isfinite(good[6]))
    bad = P.copy()
    i = int(table.parts[2][5])
    bad[i, i] = -1.0
    fb, _, _, _, _, _, value = run_terms(bad, a, table, device)
    info = fb.info.tolist()
    assert info[2] != 0 and [info[0], info[1], info[3]] == [0, 0, 0]
    assert bool(torch.isnan(value))


# ---- the golden model cases ---------------------------------------------------------------------------------------------------------
def build_model(case, objective="kfold", inputs=None, folds=None):
    x, y = maker.case_inputs(case) if inputs is None else inputs
    ls = np.asarray(case["length_scales"], dtype=np.float64) if case["ARD"] else float(case["length_scales"][0])
    k = getattr(kernels, case["kind"])(case["d"], variance=float(case["variance"]), length_scales=ls, ARD=bool(case["ARD"]))
    mean = None if case["mean"] is None else mean_functions.Constant(case["dy"], torch.tensor(case["mean"], dtype=torch.float64))
    extra = dict(folds=maker.case_folds(case) if folds is None else folds) if objective == "kfold" else {}
    m = GPR(x, y, k, mean_function=mean, likelihood=likelihoods.Gaussian(variance=float(case["noise"])), objective=objective, **extra)
    m.cuda()
    return m


def arr(case, key):
    return GOLD["%s__%s" % (case["name"], key)]


def grads_of(m):
    return [p.grad.detach().clone() for p in m.parameters() if p.grad is not None]


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
    mean, var = m.kfold_predict()
    assert mean.shape == (case["n"], case["dy"]) and var.shape == (case["n"], case["dy"]) and not mean.requires_grad
    em, ev = xr.abs_err(mean, arr(case, "mean")), xr.abs_err(var, arr(case, "var"))
    print("   kfold_predict: mean %.2e (tol %.1e) var %.2e (tol %.1e)" % (em, xr.tol(e["mean"], "mean"), ev, xr.tol(e["var"], "var")))
    assert em <= xr.tol(e["mean"], "mean") and ev <= xr.tol(e["var"], "var")
    # ... and, for the first and the last fold, against models that really never saw the fold
    off, idx = arr(case, "folds_off"), arr(case, "folds_idx")
    for tag, f in (("first", 0), ("last", len(off) - 2)):
        I = idx[off[f]:off[f + 1]]
        rm = xr.abs_err(mean[I], arr(case, "refit_%s_mean" % tag))
        rv = xr.abs_err(var[I, 0], arr(case, "refit_%s_var" % tag))
        print("   kfold_predict vs the refit without the %s fold (%d points): mean %.2e var %.2e" % (tag, I.size, rm, rv))
        assert rm <= xr.tol(e["mean"], "mean") and rv <= xr.tol(e["var"], "var")
    # no priors: the objective is the loss's negative, bit for bit, and log_likelihood() is still the LML
    assert torch.equal(m.kfold_log_predictive(), -loss.detach())
    lml = build_model(case, objective="lml")
    assert torch.equal(m.log_likelihood(), lml.log_likelihood()) and not torch.equal(m.log_likelihood(), m.kfold_log_predictive())


# ---- the dense route ------------------------------------------------------------------------------------------------------------------
def test_sum_of_two_rbf_is_one_rbf(device):
    """GPR(Rbf(v1) + Rbf(v2), objective="kfold") with one length scale is the model Rbf(v1 + v2) (_ops.DenseKFoldLik): value,
    gradients and predictions against the oracle at v = v1 + v2, the raw-variance and raw-length-scale gradients split as v1 / v
    and v2 / v."""
    n, d, v1, v2, ell, noise = 150, 2, 0.9, 0.5, 0.8, 0.05
    x, y = rng.make_regression(n, d, 1, seed=241)
    folds = shuffled(n, [40, 37, 41, 32], 243)
    ref, t64 = ko.make_pair(x, y, "Rbf", v1 + v2, ell, noise, folds=folds)
    loss64, g64 = t64.loss_grads_with_mean()
    want = ref.loss_grads()
    e_loss, e_grad = xr.rel_err(loss64, ref.loss()), max(xr.rel_err(a, b) for a, b in zip(g64, want))
    k1, k2 = kernels.Rbf(d, variance=v1, length_scales=ell), kernels.Rbf(d, variance=v2, length_scales=ell)
    m = GPR(x, y, k1 + k2, likelihood=likelihoods.Gaussian(variance=noise), objective="kfold", folds=folds)
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
    mean, var = m.kfold_predict()
    wm, wv = ref.kfold_predict()
    assert xr.abs_err(mean, wm) <= xr.tol(xr.abs_err(t64.kfold_predict()[0], wm), "mean")
    assert xr.abs_err(var, wv) <= xr.tol(xr.abs_err(t64.kfold_predict()[1], wv), "var")


# ---- determinism ------------------------------------------------------------------------------------------------------------------------
def test_same_call_same_bits_and_int_k_is_its_partition(device):
    case = CASES["exp_203x1_k6"]
    runs = []
    for folds in (6, 6, [np.asarray(p) for p in np.array_split(np.arange(203), 6)]):
        m = build_model(case, folds=folds)
        loss = m.loss()
        loss.backward()
        runs.append([loss.detach()] + grads_of(m) + list(m.kfold_predict()))
    for other in runs[1:]:
        assert len(other) == len(runs[0]) and all(torch.equal(a, b) for a, b in zip(runs[0], other))
    # ... and twice on ONE model (its reusable factor buffer holds the first call's factor)
    m = build_model(case)
    first = m.loss()
    first.backward()
    g1 = grads_of(m)
    for p in m.parameters():
        p.grad = None
    second = m.loss()
    second.backward()
    assert torch.equal(first.detach(), second.detach()) and all(torch.equal(a, b) for a, b in zip(g1, grads_of(m)))


# ---- fitting ----------------------------------------------------------------------------------------------------------------------------
FIT = dict(name="fit_96", kind="Rbf", n=96, d=2, dy=1, ARD=False, variance=1.3, length_scales=[0.8], noise=0.05, mean=None, seed=411, folds=4)


def test_adam_follows_the_fp64_statement(device):
    """10 Adam steps at n = 96, k = 4 against KFoldTorch's trajectory, as tests/test_gpu_loo.py holds its own: FLOOR["loss"] per step"""
    m = build_model(FIT)
    with quiet():
        losses, _ = m.optimize(method="Adam", max_iter=10, learning_rate=0.05, verbose=False)
    _, t64 = maker.build(FIT)
    want = t64.optimize_adam(max_iter=10, learning_rate=0.05)
    assert len(losses) == 10
    for got, w in zip(losses, want):
        print("adam: %.12f vs %.12f" % (got, w))
        assert xr.rel_err(got, w) <= xr.FLOOR["loss"]


def test_scipy_lbfgsb_lowers_the_loss(device):
    m = build_model(FIT)
    first = m.loss().item()
    with quiet():
        res = m.optimize(method="L-BFGS-B", max_iter=5, verbose=False)
    assert np.isfinite(res.fun) and res.fun < first


def test_a_noise_prior_enters_the_loss_once(device):
    m = build_model(FIT)
    plain = m.loss().detach()
    prior = torch.distributions.Gamma(torch.tensor(2.0, dtype=torch.float64, device=device), torch.tensor(10.0, dtype=torch.float64, device=device))
    m.likelihood.variance.prior = prior
    with_prior = m.loss()
    lp = prior.log_prob(m.likelihood.variance.transform()).sum().detach()
    assert lp.item() != 0.0 and torch.equal(with_prior.detach(), -(-plain + lp))
    with_prior.backward()
    assert m.likelihood.variance.grad is not None and bool(torch.isfinite(m.likelihood.variance.grad).all())


def test_capture_falls_back_to_the_ordinary_loop(device):
    m, m2 = build_model(FIT), build_model(FIT)
    assert not m._can_capture("Adam") and build_model(FIT, objective="lml")._can_capture("Adam")
    with quiet():
        captured, _ = m.optimize(method="Adam", max_iter=3, verbose=False, capture=True)
        ordinary, _ = m2.optimize(method="Adam", max_iter=3, verbose=False)
    assert np.array_equal(captured, ordinary)


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


def test_multi_start_runs_kfold_models_one_by_one(device):
    """two ordinary restarts and two objective="kfold" models in one multi_start_optimize: the ordinary two get, bit for bit, what a
    call without the others gives them; each k-fold model gets what its own optimize() gives."""
    inputs = tuple(torch.tensor(t) for t in maker.case_inputs(FIT))
    objs = ["lml", "kfold", "lml", "kfold"]
    ms, twins = restarts(FIT, objs, inputs), restarts(FIT, objs, inputs)
    with quiet():
        mixed, _ = multi_start_optimize(ms, method="Adam", max_iter=3, verbose=False, learning_rate=0.05)
        alone, _ = multi_start_optimize([twins[0], twins[2]], method="Adam", max_iter=3, verbose=False, learning_rate=0.05)
        own = [twins[i].optimize(method="Adam", max_iter=3, verbose=False, learning_rate=0.05)[0] for i in (1, 3)]
    assert np.array_equal(mixed[[0, 2]], alone) and np.array_equal(mixed[1], own[0]) and np.array_equal(mixed[3], own[1])
    for got, want in zip(ms, twins):
        assert all(torch.equal(p, q) for p, q in zip(state(got), state(want)))
    assert not np.array_equal(mixed[1], mixed[0])


def test_batched_loss_and_grad_evaluates_kfold_models_by_themselves(device):
    inputs = tuple(torch.tensor(t) for t in maker.case_inputs(FIT))
    objs = ["kfold", "lml", "kfold", "lml"]
    ms, single = restarts(FIT, objs, inputs), restarts(FIT, objs, inputs)
    out = batched_loss_and_grad(ms)
    for m, s, o in zip(ms, single, out):
        loss = s.loss()
        loss.backward()
        assert torch.equal(o, loss.detach())
        assert all(torch.equal(p.grad, q.grad) for p, q in zip(m.parameters(), s.parameters()) if q.grad is not None)


def test_default_objective_keeps_its_bits_after_a_kfold_evaluation(device):
    """a default-objective model evaluated after a k-fold model on the same data carries the bits of one evaluated alone"""
    case = CASES["matern52_300x17_shuffled"]
    inputs = tuple(torch.tensor(t) for t in maker.case_inputs(case))
    alone = build_model(case, objective="lml", inputs=inputs)
    la = alone.loss()
    la.backward()
    kf = build_model(case, inputs=inputs)
    lk = kf.loss()
    lk.backward()
    after = build_model(case, objective="lml", inputs=inputs)
    lb = after.loss()
    lb.backward()
    assert torch.equal(la.detach(), lb.detach()) and not torch.equal(la.detach(), lk.detach())
    pairs = [(p.grad, q.grad) for p, q in zip(alone.parameters(), after.parameters()) if p.grad is not None or q.grad is not None]
    assert len(pairs) >= 3 and all(torch.equal(g, h) for g, h in pairs)
    for a, b in zip(alone.predict_y(alone.X[:5]), after.predict_y(after.X[:5])):
        assert torch.equal(a, b)
