"""The autograd nodes of the inducing-point models (VFE, FITC, SVGP) on both kernel adapters: which gradient lands in which
slot when a parameter is frozen, and that no node can be differentiated twice.

A node takes the differentiable kernel tensors as trailing arguments and returns their gradients by position.  Freezing one
kernel parameter shortens that list for a composite kernel (the adapter differentiates the raw parameters that require a
gradient) and leaves it as it is for a native kind (constrained variance and length-scales, whatever requires a gradient);
freezing Z changes nothing in the list.  In every case the arithmetic that produces the OTHER gradients is the same sequence
of launches on the same operands, so they -- and the loss -- are compared with torch.equal, not to a tolerance."""
import numpy as np
import pytest
import torch

from gptorch_amd import kernels, likelihoods, rng
from gptorch_amd.models import FITC, SVGP, VFE, sparse_gpr

pytestmark = pytest.mark.gpu

D, DY = 3, 2
MODELS = {"VFE": VFE, "FITC": FITC, "SVGP": SVGP}
# kernel -> (constructor, the one kernel variance that is frozen)
KERNELS = {
    "matern52_ard": (lambda: kernels.Matern52(D, variance=1.3, length_scales=np.array([0.9, 1.4, 1.1]), ARD=True), "kernel.variance"),
    "rbf_plus_linear": (lambda: kernels.Rbf(D, variance=1.2, length_scales=1.1) + kernels.Linear(D, variance=0.4), "kernel.kern1.variance"),
}


def build(model, kern, n, m, frozen=None):
    x, y = rng.make_regression(n, D, DY, seed=11)
    z = rng.normal(12, (m, D))
    np.random.seed(3)                                                        # SVGP's constructor draws its initial posterior's rows
    mdl = MODELS[model](x, y, KERNELS[kern][0](), inducing_points=z.copy(), likelihood=likelihoods.Gaussian(variance=0.1))
    if frozen is not None:
        dict(mdl.named_parameters())[frozen].requires_grad_(False)
    mdl.cuda()
    return mdl


def loss_and_grads(mdl):
    loss = mdl.loss()
    loss.backward()
    return loss.detach(), {k: p.grad for k, p in mdl.named_parameters()}


@pytest.mark.parametrize("chunk_rows", [None, 64], ids=["one_chunk", "two_chunks"])
@pytest.mark.parametrize("kern", list(KERNELS))
@pytest.mark.parametrize("model", list(MODELS))
def test_gradient_slots_under_frozen_parameters(device, monkeypatch, model, kern, chunk_rows):
    """N = 150, M = 20, d = 3, dy = 2: an all-trainable model against copies with (a) one kernel variance, (b) Z frozen."""
    if chunk_rows is not None:
        monkeypatch.setattr(sparse_gpr, "CHUNK_ROWS", chunk_rows)
        assert [r for _, r in sparse_gpr._chunks(150, sparse_gpr._chunk_rows(150))] == [128, 22]           # (a chunk is a whole number of 128-row leaves)
    loss0, g0 = loss_and_grads(build(model, kern, 150, 20))
    trainable = [k for k, g in g0.items() if g is not None]
    assert {KERNELS[kern][1], "Z", "likelihood.variance"} <= set(trainable)
    for frozen in (KERNELS[kern][1], "Z"):
        loss1, g1 = loss_and_grads(build(model, kern, 150, 20, frozen=frozen))
        assert g1[frozen] is None, (frozen, "has a gradient")
        assert torch.equal(loss1, loss0), (frozen, loss1.item(), loss0.item())
        for k in trainable:
            if k != frozen:
                assert g1[k] is not None and g1[k].shape == g0[k].shape, (frozen, k)
                assert torch.equal(g1[k], g0[k]), (frozen, k, (g1[k] - g0[k]).abs().max().item())


@pytest.mark.parametrize("model", list(MODELS))
def test_double_backward_raises(device, model):
    """Every node's backward is closed-form arithmetic on detached values: a second derivative taken through it would be that of
    `g * constant`, not the bound's Hessian, so every node is @once_differentiable (as every other node of the package is).

    What that decorator guards is a backward whose INCOMING gradient requires a gradient: then its outputs are tied to a node
    that raises when it is differentiated.  Under loss() alone the incoming gradient is the constant -1, and the gradients that
    come straight out of a node (Z's: no transform in between) carry no graph at all -- differentiating them raises because
    there is nothing to differentiate, with or without the decorator.  So both are checked: (1) the plain recipe on Z's
    gradient, (2) the loss scaled by a differentiable weight, where a node without the decorator would return numbers."""
    mdl = build(model, "matern52_ard", 60, 8)
    params = [p for p in mdl.parameters() if p.requires_grad]
    names = [k for k, p in mdl.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(mdl.loss(), params, create_graph=True)
    with pytest.raises(RuntimeError):
        grads[names.index("Z")].sum().backward()
    weight = torch.ones((), dtype=torch.float64, device=device, requires_grad=True)
    grads = torch.autograd.grad(mdl.loss() * weight, params, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        sum(g.sum() for g in grads).backward()
