"""Leave-one-out GPR in lock step on the GPU: the three gpn_loo_*_batched entry points against their single calls row by row (the
same kernels with the model on the grid's y dimension: equal BITS are asked, torch.equal), groups of objective="loo" models through
batched_loss_and_grad and multi_start_optimize against each model's own loss().backward() / optimize(), the golden cases as groups,
a failing model's replay, priors, a mixed list, a backward that outlives its buffers, and the tests that fail without the feature.

Comparisons are torch.equal unless said otherwise.  Mean-function parameters: rtol = atol = 1e-12, the allowance
tests/test_gpu_lockstep_fit.py gives the LML groups (their gradient is a sum over a stacked residual gradient, which torch adds up in
another order than over one model's).  Golden cases: tests/_xref.tol of the stored e64, as tests/test_gpu_loo.py."""
import numpy as np
import pytest
import torch

from gptorch_amd import _native, _ops, kernels, likelihoods, rng
from gptorch_amd.models import GPR, LaplaceGP, _lockstep, _loo_lockstep, batched_loss_and_grad, multi_start_optimize
from tests import _xref as xr
from tests.golden import make_loo_golden as maker
from tests.test_gpu_loo import CASES, GRAD_KINDS, arr, build_model, cuda, lower_buffer, quiet, restarts, spd

pytestmark = pytest.mark.gpu

NAN = float("nan")
EDGE_N = [1, 63, 64, 65, 129, 257]
BATCHES = [1, 2, 3]


def nan_buffer(*shape):
    return torch.full(shape, NAN, dtype=torch.float64, device="cuda")


def stream():
    return _ops._stream(torch.device("cuda", torch.cuda.current_device()))


# ---- the entry points, row by row ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("n", EDGE_N)
def test_terms_batched_rows_are_the_single_calls(device, n, batch):
    """every model's P and a^T sit in NaN-filled buffers, a model stride larger than the block; the outputs start NaN-filled and only
    [dy, n] / [n] of each model's block changes."""
    lib = _native.lib()
    for dy in (1, 5):
        ld = int(lib.gpn_factor_ld(n, dy))
        rows = _ops.round_up(n, 64)
        sK, sAt = rows * ld + 6, 16 * ld + 10                   # gaps between the models' blocks
        Kinv, at = nan_buffer(batch * sK), nan_buffer(batch * sAt)
        qrows = 8
        sQt = qrows * ld + 2
        qt = nan_buffer(batch * sQt)
        singles = []
        for b in range(batch):
            Kb = Kinv[b * sK:b * sK + rows * ld].view(rows, ld)
            Kb.diagonal()[:n] = cuda(0.2 + 3.0 * rng.uniform(100 + n + dy + 7 * b, n))                  # only the diagonal is read
            ab = at[b * sAt:b * sAt + 16 * ld].view(16, ld)
            ab[:dy, :n] = cuda(rng.normal(200 + n + dy + 7 * b, (dy, n)))
            singles.append(_ops.loo_terms(Kb, ab[:dy, :n], n, dy))
        var, rootd, value = nan_buffer(batch, n), nan_buffer(batch, n), nan_buffer(batch)
        work = nan_buffer(max(1, int(lib.gpn_loo_terms_batched_work_bytes(n, batch)) // 8))
        st = lib.gpn_loo_terms_batched(stream(), batch, n, dy, _ops._ptr(Kinv), ld, sK, _ops._ptr(at), ld, sAt, _ops._ptr(work), work.numel() * 8,
                                       _ops._ptr(qt), ld, sQt, _ops._ptr(var), _ops._ptr(rootd), _ops._ptr(value))
        assert st == 0
        untouched = torch.ones_like(qt, dtype=torch.bool)
        for b, (q1, v1, r1, val1) in enumerate(singles):
            qb = qt[b * sQt:b * sQt + qrows * ld].view(qrows, ld)
            assert torch.equal(qb[:dy, :n], q1) and torch.equal(var[b], v1) and torch.equal(rootd[b], r1) and torch.equal(value[b], val1), (dy, b)
            untouched[b * sQt:b * sQt + qrows * ld].view(qrows, ld)[:dy, :n] = False
        assert bool(torch.isnan(qt[untouched]).all())
        # NULL outputs leave the others' bits alone
        value2 = nan_buffer(batch)
        st = lib.gpn_loo_terms_batched(stream(), batch, n, dy, _ops._ptr(Kinv), ld, sK, _ops._ptr(at), ld, sAt, _ops._ptr(work), work.numel() * 8,
                                       None, 0, 0, None, None, _ops._ptr(value2))
        assert st == 0 and torch.equal(value2, value)


def test_terms_batched_one_bad_precision_stays_in_its_model(device):
    """p_i = 0 in ONE model: that model's point and value are NaN, the other models' rows keep the bits of their single calls."""
    n, dy, batch = 300, 2, 3
    Kinv = torch.zeros(batch, n, n, dtype=torch.float64, device=device)
    at = cuda(rng.normal(8, (batch, dy, n)))
    for b in range(batch):
        Kinv[b].diagonal().copy_(cuda(0.2 + 3.0 * rng.uniform(7 + b, n)))
    good = [_ops.loo_terms(Kinv[b], at[b], n, dy) for b in range(batch)]
    Kinv[1, 70, 70] = 0.0
    qt = nan_buffer(batch, dy, n)
    var, rootd, value = _ops.loo_terms_batched(batch, n, dy, Kinv, n, n * n, at, n, dy * n, Kinv.device, qt=qt, ldqt=n, sQt=dy * n)
    assert bool(torch.isnan(value[1])) and bool(torch.isnan(var[1, 70])) and bool(torch.isnan(rootd[1, 70])) and bool(torch.isnan(qt[1, :, 70]).all())
    keep = torch.arange(n, device=device) != 70
    assert torch.equal(qt[1][:, keep], good[1][0][:, keep]) and torch.equal(var[1][keep], good[1][1][keep]) and torch.equal(rootd[1][keep], good[1][2][keep])
    for b in (0, 2):
        assert torch.equal(qt[b], good[b][0]) and torch.equal(var[b], good[b][1]) and torch.equal(rootd[b], good[b][2]) and torch.equal(value[b], good[b][3])


@pytest.mark.parametrize("odd_ld", [False, True], ids=["factor_ld", "odd_ld"])
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("n", EDGE_N)
def test_scale_batched_rows_are_the_single_calls(device, n, batch, odd_ld):
    """S_b on BOTH triangles from each model's lower triangle in a NaN-filled buffer; a sentinel fill shows that nothing outside
    [n, n] of a model's block is written, the gap between two blocks included.  odd_ld (and the odd model stride that goes with it)
    rules the 16-byte loads out."""
    lib = _native.lib()
    ld, rows = int(lib.gpn_factor_ld(n, 0)) + (1 if odd_ld else 0), int(lib.gpn_factor_rows(n, 0))
    krows = _ops.round_up(n, 64)
    sK, sS = krows * ld + (3 if odd_ld else 4), rows * ld + 5
    Kinv = nan_buffer(batch * sK)
    rootd = cuda(0.1 + rng.uniform(400 + n, batch * n).reshape(batch, n))
    sentinel = -7.25
    S = torch.full((batch * sS,), sentinel, dtype=torch.float64, device=device)
    singles = []
    for b in range(batch):
        Kb = Kinv[b * sK:b * sK + krows * ld].view(krows, ld)
        Kb.copy_(lower_buffer(spd(n, 300 + n + b), ld, device))
        T = torch.full((rows, ld), sentinel, dtype=torch.float64, device=device)
        singles.append(_ops.loo_scale(Kb, rootd[b], n, T))
    _ops.loo_scale_batched(batch, n, Kinv, ld, sK, rootd, S, ld, sS)
    for b in range(batch):
        assert torch.equal(S[b * sS:b * sS + rows * ld].view(rows, ld), singles[b]), b          # the block with its sentinels
        assert bool((S[b * sS + rows * ld:(b + 1) * sS] == sentinel).all())                      # the gap


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("n", EDGE_N)
def test_grad_batched_rows_are_the_single_calls(device, n, batch):
    """d = 17 crosses the 16-coordinate staging, dy = 5 the 4-at-a-time staging of a^T / w^T; one length scale and ARD; shared points
    and every model's own; Q's lower triangle, a^T and w^T in NaN-filled buffers with gaps between the models."""
    lib = _native.lib()
    i = EDGE_N.index(n) + batch
    for d in (1, 17):
        for dy in (1, 5):
            for ard in (False, True):
                for shared in (False, True):
                    i += 1
                    check_grad_batched(lib, GRAD_KINDS[i % 6], n, batch, d, dy, ard, shared)


@pytest.mark.parametrize("kind", GRAD_KINDS)
def test_grad_batched_every_kind(device, kind):
    check_grad_batched(_native.lib(), kind, 129, 3, 3, 2, True, False)


def check_grad_batched(lib, kind, n, batch, d, dy, ard, shared):
    nls = d if ard else 1
    ldq = int(lib.gpn_factor_ld(n, dy))
    qrows = _ops.round_up(n, 64)
    sQ, sV = qrows * ldq + 8, 8 * ldq + 6                        # the models' strides: larger than the blocks
    X = cuda(rng.normal(1000 + 31 * n + d, (n, d) if shared else (batch, n, d)) * (1.0 / np.sqrt(d)))
    var = cuda(1.3 + 0.2 * np.arange(batch))
    ls = cuda(0.7 + 0.6 * rng.uniform(2000 + n + d, batch * nls).reshape(batch, nls))
    Q, at, wt = nan_buffer(batch * sQ), nan_buffer(batch * sV), nan_buffer(batch * sV)
    singles = []
    for b in range(batch):
        Qb = Q[b * sQ:b * sQ + qrows * ldq].view(qrows, ldq)
        Qb.copy_(lower_buffer(spd(n, 500 + n + d + b), ldq, "cuda"))
        ab, wb = (t[b * sV:b * sV + 8 * ldq].view(8, ldq) for t in (at, wt))
        ab[:dy, :n] = cuda(rng.normal(600 + n + dy + b, (dy, n)))
        wb[:dy, :n] = cuda(rng.normal(700 + n + dy + b, (dy, n)))
        singles.append(_ops.loo_grad(kind, X if shared else X[b], var[b:b + 1], ls[b], Qb, ab[:dy, :n], wb[:dy, :n]))
    out = nan_buffer(batch + 1, 2 + nls)                          # one row more: it stays NaN
    work = nan_buffer(max(1, int(lib.gpn_loo_grad_batched_work_bytes(n, nls, batch)) // 8))
    st = lib.gpn_loo_grad_batched(stream(), _ops.KINDS[kind], batch, _ops._ptr(X), 0 if shared else n * d, n, d, _ops._ptr(var), _ops._ptr(ls), nls,
                                  _ops._ptr(Q), ldq, sQ, _ops._ptr(at), ldq, sV, _ops._ptr(wt), ldq, sV, dy, _ops._ptr(work), work.numel() * 8,
                                  _ops._ptr(out))
    assert st == 0
    for b in range(batch):
        assert torch.equal(out[b], singles[b]), (kind, n, batch, d, dy, ard, shared, b, out[b], singles[b])
    assert bool(torch.isnan(out[batch]).all())
    # the wrapper: the same rows
    got = _ops.loo_grad_batched(kind, X, var, ls, Q, ldq, sQ, at, ldq, sV, wt, ldq, sV, dy)
    assert torch.equal(got, out[:batch])


def test_n_zero_zeroes_value_and_out(device):
    lib = _native.lib()
    one = cuda([1.0])
    value, out = nan_buffer(3), nan_buffer(3, 3)
    assert lib.gpn_loo_terms_batched(stream(), 3, 0, 1, _ops._ptr(one), 0, 0, _ops._ptr(one), 0, 0, None, 0, None, 0, 0, None, None, _ops._ptr(value)) == 0
    assert lib.gpn_loo_grad_batched(stream(), 0, 3, _ops._ptr(one), 0, 0, 1, _ops._ptr(one), _ops._ptr(one), 1, _ops._ptr(one), 0, 0, _ops._ptr(one), 0, 0,
                                    _ops._ptr(one), 0, 0, 1, None, 0, _ops._ptr(out)) == 0
    assert bool((value == 0).all()) and bool((out == 0).all())


# ---- groups of models --------------------------------------------------------------------------------------------------------------
def grads_of(m):
    return [None if p.grad is None else p.grad.detach().clone() for p in m.parameters()]


def own_evaluation(ms):
    """each model's own loss().backward(): [(loss, grads)], the gradients cleared again"""
    out = []
    for m in ms:
        loss = m.loss()
        loss.backward()
        out.append((loss.detach().clone(), grads_of(m)))
        m.zero_grad()
    return out


def assert_own_bits(ms, losses, want):
    for i, m in enumerate(ms):
        assert torch.equal(losses[i], want[i][0]), (i, losses[i], want[i][0])
        mean_ids = {id(p) for p in m.mean_function.parameters()}
        for p, gw in zip(m.parameters(), want[i][1]):
            assert (p.grad is None) == (gw is None)
            if gw is None:
                continue
            if id(p) in mean_ids:
                assert torch.allclose(p.grad, gw, rtol=1e-12, atol=1e-12), (i, p.grad, gw)
            else:
                assert torch.equal(p.grad, gw), (i, p.grad, gw)


def case_restarts(name, count=3):
    case = CASES[name]
    inputs = tuple(torch.tensor(t) for t in maker.case_inputs(case))
    return restarts(case, ["loo"] * count, inputs)


def loo_plan(ms):
    plan = _lockstep._plan_groups(ms)
    assert all(isinstance(grp, _lockstep.Group) for grp in plan)
    return plan


@pytest.mark.parametrize("name", ["rbf_300x2", "matern52_ard_257x3", "exp_513x2_dy5"])
def test_group_of_restarts_gets_each_models_own_bits(device, name):
    """three restarts of a golden case (matern52_ard_257x3: ARD, dy = 2, a trainable Constant mean; exp_513x2_dy5: n = 513 takes the
    strided n > 256 inversion of gpn_lml_kinv_batched)"""
    ms = case_restarts(name)
    want = own_evaluation(ms)
    plan = loo_plan(ms)
    assert [grp.family.name for grp in plan] == ["loo"] and plan[0].key.objective == "loo" and plan[0].indices == [0, 1, 2]
    losses = batched_loss_and_grad(ms)
    assert_own_bits(ms, losses, want)
    # ... and again from the cached buffers (the second call of a search)
    for m in ms:
        m.zero_grad()
    assert_own_bits(ms, batched_loss_and_grad(ms, _plan=plan), want)


def test_group_on_shared_tensors(device):
    """restarts that hold the SAME device tensors: the points and the residuals go in once (sX = 0)"""
    case = CASES["rbf_300x2"]
    inputs = tuple(torch.tensor(t).cuda() for t in maker.case_inputs(case))
    ms = restarts(case, ["loo"] * 3, inputs)
    assert ms[1].X.data_ptr() == ms[0].X.data_ptr()
    want = own_evaluation(ms)
    assert_own_bits(ms, batched_loss_and_grad(ms), want)


@pytest.mark.parametrize("name", list(CASES))
def test_golden_case_as_a_group_of_two(device, name):
    case = CASES[name]
    e = case["e64"]
    ms = [build_model(case), build_model(case)]
    assert [grp.family.name for grp in loo_plan(ms)] == ["loo"]
    losses = batched_loss_and_grad(ms)
    for m, loss in zip(ms, losses):
        err = xr.rel_err(loss.item(), case["loss"])
        print("%s: loss rel err %.2e (tol %.1e)" % (name, err, xr.tol(e["loss"], "loss")))
        assert loss.shape == (1,) and err <= xr.tol(e["loss"], "loss")
        grads = [("variance", m.kernel.variance), ("length_scales", m.kernel.length_scales), ("noise", m.likelihood.variance)]
        if case["mean"] is not None:
            grads.append(("mean", m.mean_function.val))
        for gname, p in grads:
            want = arr(case, "grad_" + gname)
            gerr = xr.rel_err(p.grad.cpu().numpy().reshape(want.shape), want)
            print("   d/d%-14s rel err %.2e (tol %.1e)" % (gname, gerr, xr.tol(e["grad"], "grad")))
            assert gerr <= xr.tol(e["grad"], "grad"), gname


def test_a_failing_model_is_replayed_alone(device):
    """one model of four has duplicated rows and a raw noise of -80 (tests/test_gpu_lockstep_fit.py
    test_lockstep_backward_replays_the_ladder_per_failing_model): the forward replays THAT model through the jitter ladder into a
    private state, the backward runs on it; all four match their own evaluations."""
    n, d = 600, 2
    x, y = rng.make_regression(n, d, 1, seed=21)
    xdup = np.array(x)
    xdup[300:] = xdup[:300]
    ms = []
    for b in range(4):
        m = GPR(xdup if b == 2 else x, y, kernels.Rbf(d, variance=1.0 + 0.1 * b, length_scales=1.3), likelihood=likelihoods.Gaussian(variance=0.03),
                objective="loo")
        m.cuda()
        if b == 2:
            m.likelihood.variance.data.fill_(-80.0)
        ms.append(m)
    want = own_evaluation(ms)
    assert ms[2]._holder["factor"].jitter_rung >= 0
    plan = loo_plan(ms)
    (group,) = plan
    key, g = group.key, group.indices
    assert g == [0, 1, 2, 3] and key.objective == "loo" and group.family.name == "loo"
    losses = batched_loss_and_grad(ms, _plan=plan)
    replayed = _lockstep._BATCH_BUFFERS[(key, 4)]["loo_replayed"]
    assert list(replayed) == [2] and replayed[2] >= 0 and replayed[2] == ms[2]._holder["factor"].jitter_rung
    assert_own_bits(ms, losses, want)


def test_a_noise_prior_enters_its_models_loss_once(device):
    ms = case_restarts("rbf_300x2")
    plain = [l.clone() for l in batched_loss_and_grad(ms)]
    for m in ms:
        m.zero_grad()
    prior = torch.distributions.Gamma(torch.tensor(2.0, dtype=torch.float64, device=device), torch.tensor(10.0, dtype=torch.float64, device=device))
    ms[1].likelihood.variance.prior = prior
    want = own_evaluation(ms)
    plan = loo_plan(ms)
    assert plan[0].priors is True                                 # the group's "has priors" flag
    losses = batched_loss_and_grad(ms, _plan=plan)
    lp = prior.log_prob(ms[1].likelihood.variance.transform()).sum().detach()
    assert lp.item() != 0.0 and torch.equal(losses[1], -(-plain[1] + lp))
    assert torch.equal(losses[0], plain[0]) and torch.equal(losses[2], plain[2])
    assert_own_bits(ms, losses, want)


def mixed_list():
    case = CASES["rbf_300x2"]
    inputs = tuple(torch.tensor(t) for t in maker.case_inputs(case))
    a, b, c, e = restarts(case, ["lml", "loo", "lml", "loo"], inputs)
    x2, y2 = rng.make_regression(200, 2, 1, seed=31)
    other = GPR(x2, y2, kernels.Rbf(2, variance=1.1, length_scales=0.9), likelihood=likelihoods.Gaussian(variance=0.05), objective="loo")
    comp = GPR(x2, y2, kernels.Rbf(2, variance=0.9, length_scales=0.8) + kernels.Rbf(2, variance=0.5, length_scales=1.7),
               likelihood=likelihoods.Gaussian(variance=0.05), objective="loo")
    labels = (np.asarray(y2) > 0).astype(np.float64)
    laps = [LaplaceGP(x2, labels, kernels.Rbf(2, variance=1.0 + 0.3 * k, length_scales=1.0), likelihoods.Bernoulli("probit")) for k in range(2)]
    ms = [a, b, other, c, comp, laps[0], e, laps[1]]
    for m in ms:
        m.cuda()
    return ms


def test_a_mixed_list(device):
    """2 LML, 2 LOO, 1 LOO of another n, 1 composite-kernel LOO and 2 LaplaceGP models in one call; every model's own bits come from
    a twin list built the same way (a LaplaceGP model starts its second search from the first one's mode)"""
    want = own_evaluation(mixed_list())
    ms = mixed_list()
    plan = loo_plan(ms)
    assert [grp.family.name for grp in plan] == ["lml", "loo", "laplace"]
    by_objective = {grp.key.objective: grp.indices for grp in plan[:2]}
    assert by_objective == {"lml": [0, 3], "loo": [1, 6]}
    assert plan[2].indices == [5, 7]
    losses = batched_loss_and_grad(ms, _plan=plan)
    assert_own_bits(ms, losses, want)


# ---- multi_start_optimize -------------------------------------------------------------------------------------------------------------
def state(m):
    return [p.detach().clone() for p in m.parameters()]


@pytest.mark.parametrize("stacked", [None, True])
def test_multi_start_adam_follows_each_models_own_optimize(device, stacked):
    """LOO groups take the bitwise mode at every size: their own optimiser objects, one lock-step evaluation per iteration"""
    ms, twins = case_restarts("rbf_300x2"), case_restarts("rbf_300x2")
    with quiet():
        got, _ = multi_start_optimize(ms, method="Adam", max_iter=3, verbose=False, learning_rate=0.05, stacked=stacked)
        own = [t.optimize(method="Adam", max_iter=3, verbose=False, learning_rate=0.05)[0] for t in twins]
    for i, (m, t) in enumerate(zip(ms, twins)):
        assert np.array_equal(got[i], np.asarray(own[i])), i
        assert all(torch.equal(p, q) for p, q in zip(state(m), state(t))), i
    assert not np.array_equal(got[0], got[1])


def test_multi_start_scipy_reaches_the_group(device, monkeypatch):
    """L-BFGS-B, 5 iterations: every round of function evaluations that still covers at least two restarts is ONE lock-step
    evaluation (a round that covers a single restart -- the others have finished -- is that model's own loss()); each restart's
    result is its own run's."""
    ms, twins = case_restarts("rbf_300x2"), case_restarts("rbf_300x2")
    with quiet():
        own = [t.optimize(method="L-BFGS-B", max_iter=5, verbose=False) for t in twins]
    calls = {"group": [], "single": 0}
    group_init, single_terms = _ops.LooGroupState.__init__, _ops.loo_terms

    def counted_group(self, kind, X, R, variance, *rest):
        calls["group"].append(int(variance.numel()))
        group_init(self, kind, X, R, variance, *rest)

    def counted_single(*a, **k):
        calls["single"] += 1
        return single_terms(*a, **k)

    monkeypatch.setattr(_ops.LooGroupState, "__init__", counted_group)
    monkeypatch.setattr(_ops, "loo_terms", counted_single)
    with quiet():
        res, _ = multi_start_optimize(ms, method="L-BFGS-B", max_iter=5, verbose=False)
    for r, o in zip(res, own):
        assert r.fun == o.fun and np.array_equal(r.x, o.x) and r.nfev == o.nfev
    # the first round covers all three; every evaluation is accounted for by a group of its size or by a singleton's own loss()
    assert calls["group"] and calls["group"][0] == 3 and all(size >= 2 for size in calls["group"])
    assert sum(calls["group"]) + calls["single"] == sum(o.nfev for o in own)


# ---- the buffers ------------------------------------------------------------------------------------------------------------------------
def test_backward_survives_a_later_forward(device):
    """forward group A, forward group A again at other hyper-parameters (the same cached buffers), then backward the FIRST: the
    stamp has moved, the node rebuilds its state privately, and the gradients are those of the first."""
    ms = case_restarts("matern52_ard_257x3")
    want = own_evaluation(ms)
    key = loo_plan(ms)[0].key
    holder = _lockstep._batch_holder((key, len(ms)))

    def forward():
        X, R, _ = _lockstep._group_data(ms, differentiable=True, key=key)
        var, ls, nz = _lockstep._group_hypers(ms, differentiable=True)
        return _ops.BatchedGPRLooLik.apply(X, R, var, ls, nz, key.kind, holder)

    first = forward()
    with torch.no_grad():
        for m in ms:
            m.kernel.variance.data.add_(0.3)
    second = forward()
    assert not torch.equal(first.detach(), second.detach())
    with torch.no_grad():
        for m in ms:
            m.kernel.variance.data.sub_(0.3)
    (-(first + 0.0)).sum().backward()
    assert_own_bits(ms, [-(first.detach()[b:b + 1] + 0.0) for b in range(len(ms))], want)


def test_the_workspace_counts_into_the_cache_bound(device):
    _lockstep.release_batch_buffers()
    ms = case_restarts("rbf_300x2")
    batched_loss_and_grad(ms)
    n, dy, nls = 300, 1, 1
    held = _lockstep._held_bytes()
    lib = _native.lib()
    # at least the factors, the inversion's workspace and Q; at most what every model is charged (the capacity rule's figure)
    least = 3 * (8 * int(lib.gpn_factor_rows(n, dy)) * int(lib.gpn_factor_ld(n, dy)) + int(lib.gpn_lml_kinv_batched_work_bytes(n, dy, 1)) +
                 8 * _ops.round_up(n, 64) * int(lib.gpn_factor_ld(n, 0)))
    assert least <= held <= 3 * _loo_lockstep.per_model_bytes(n, dy, nls)
    _lockstep.release_batch_buffers()
    assert _lockstep._held_bytes() == 0


# ---- what fails without the feature ----------------------------------------------------------------------------------------------------
def test_the_lockstep_path_runs(device, monkeypatch):
    """with the single-model entry points patched to raise, a LOO group of three still evaluates; a singleton goes through its own
    loss() again once the patch is gone"""
    ms = case_restarts("rbf_300x2")
    want = own_evaluation(ms)

    def refuse(*a, **k):
        raise AssertionError("the single-model leave-one-out route ran")

    with monkeypatch.context() as mp:
        mp.setattr(_ops, "loo_grad", refuse)
        mp.setattr(_ops, "loo_terms", refuse)
        losses = batched_loss_and_grad(ms)
        assert_own_bits(ms, losses, want)
        with pytest.raises(AssertionError, match="single-model"):
            batched_loss_and_grad(ms[:1])
    ms[0].zero_grad()
    assert [grp for grp in loo_plan(ms[:1]) if grp.family.name in ("lml", "loo")] == []
    alone = batched_loss_and_grad(ms[:1])
    assert_own_bits(ms[:1], alone, want[:1])
