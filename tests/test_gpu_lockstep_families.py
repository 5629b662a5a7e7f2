"""One list holding every lock-step family at once (models/_lockstep.py: FAMILIES): two equal-shape models of each of stationary
LML, leave-one-out, composite-kernel, VFE, LaplaceGP and EPGP, interleaved, and one singleton that no group takes.  n = 130 (one
row block past a 128-row leaf), d = 2, dy = 1, 16 inducing points.  Every comparison is exact: the reference is each model's own
sequential evaluation on an identically built list."""
import contextlib
import io

import numpy as np
import pytest
import torch

from gptorch_amd import kernels, likelihoods, mean_functions, rng
from gptorch_amd.models import EPGP, GPR, VFE, LaplaceGP, batched_factorise, batched_log_likelihood, batched_loss_and_grad
from gptorch_amd.models import _lockstep

pytestmark = pytest.mark.gpu

N, D, M = 130, 2, 16
FAMILY_OF = ["lml", "loo", "expr", "vfe", "laplace", "ep", None, "ep", "laplace", "vfe", "expr", "loo", "lml"]     # None: the singleton


def build():
    """the mixed list, from fixed seeds: the two models of a family differ in their kernel variance"""
    x, y = rng.make_regression(N, D, 1, seed=11)
    labels = (np.asarray(y) > 0).astype(np.float64)
    seen = {}
    ms = []
    for name in FAMILY_OF:
        var = 0.8 + 0.3 * seen.setdefault(name, 0)
        seen[name] += 1
        if name in ("lml", "loo"):
            m = GPR(x, y, kernels.Rbf(D, variance=var, length_scales=1.2), likelihood=likelihoods.Gaussian(variance=0.05), objective=name)
        elif name == "expr":
            m = GPR(x, y, kernels.Linear(D, variance=var) + kernels.Rbf(D, length_scales=0.9) + kernels.Constant(D, variance=0.3),
                    likelihood=likelihoods.Gaussian(variance=0.05))
        elif name == "vfe":
            m = VFE(x, y, kernels.Rbf(D, variance=var, length_scales=1.1), inducing_points=x[:M] + 0.01 * seen[name],
                    likelihood=likelihoods.Gaussian(variance=0.05), mean_function=mean_functions.Zero(1))
        elif name == "laplace":
            m = LaplaceGP(x, labels, kernels.Rbf(D, variance=var, length_scales=1.0), likelihoods.Bernoulli("probit"))
        elif name == "ep":
            m = EPGP(x, labels, kernels.Rbf(D, variance=var, length_scales=1.0), likelihoods.Bernoulli("probit"))
        else:
            m = GPR(x, y, kernels.Matern32(D, variance=1.1, length_scales=1.3), likelihood=likelihoods.Gaussian(variance=0.05))
        m.cuda()
        ms.append(m)
    return ms


def fitted():
    """the list after two Adam steps of every model's own optimize()"""
    ms = build()
    with contextlib.redirect_stdout(io.StringIO()):
        for m in ms:
            m.optimize(method="Adam", max_iter=2, learning_rate=0.01)
    return ms


def indices_of(name):
    return [i for i, f in enumerate(FAMILY_OF) if f == name]


def test_the_plan_holds_one_group_of_each_family(device):
    plan = _lockstep._plan_groups(build())
    assert [grp.family.name for grp in plan] == ["lml", "loo", "expr", "vfe", "laplace", "ep"]
    assert all(grp.indices == indices_of(grp.family.name) and grp.priors is False for grp in plan)
    assert all(grp.family is family for grp, family in zip(plan, _lockstep.FAMILIES))


def test_log_likelihood_is_each_models_own(device):
    want = [m.log_likelihood().detach() for m in build()]
    with torch.no_grad():
        got = batched_log_likelihood(build())
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and torch.equal(g, w), (i, FAMILY_OF[i])
    assert [tuple(w.shape) for w in want] == [() if f == "vfe" else (1,) for f in FAMILY_OF]


def test_loss_and_grad_are_each_models_own(device):
    lock, alone = build(), build()
    got = batched_loss_and_grad(lock)
    for i, (g, ma, mb) in enumerate(zip(got, alone, lock)):
        loss = ma.loss()
        loss.backward()
        assert g.shape == loss.shape and torch.equal(g, loss.detach()), (i, FAMILY_OF[i])
        for p, q in zip(ma.parameters(), mb.parameters()):
            assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), (i, FAMILY_OF[i])
        assert any(q.grad is not None for q in mb.parameters()), (i, FAMILY_OF[i])


def test_factorise_seeds_the_families_that_seed_and_release_frees_everything(device):
    seeded, alone = fitted(), fitted()
    # the stationary family takes the LML and the leave-one-out models (their predictions start from the same factor); with the
    # LaplaceGP and the EPGP group: 4 + 2 + 2.  The singleton, the composite-kernel and the VFE models are left to their own _predict
    count = sum(len(grp.indices) for family in _lockstep.FAMILIES if family.seed is not None for grp in family.groups(seeded))
    assert [family.name for family in _lockstep.FAMILIES if family.seed is not None] == ["lml", "laplace", "ep"] and count == 8
    assert batched_factorise(seeded) == count
    xs = torch.tensor(rng.normal(5, (7, D))).cuda()
    for i, (ma, mb) in enumerate(zip(alone, seeded)):
        got, want = mb.predict_f(xs), ma.predict_f(xs)
        assert len(got) == len(want) == 2 and all(g.shape == w.shape and torch.equal(g, w) for g, w in zip(got, want)), (i, FAMILY_OF[i])
    batched_loss_and_grad(build())
    assert _lockstep._held_bytes() > 0
    _lockstep.release_batch_buffers()
    assert _lockstep._held_bytes() == 0
