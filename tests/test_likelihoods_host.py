"""CPU suite: the non-Gaussian likelihoods' torch route (gptorch_amd/likelihoods.py) against the 40-digit goldens of
tests/golden/make_lik_golden.py, the closed forms against the rule they replace, the rule's truncation error, and the
interface (shapes, type errors, what raises).  The fused kernel's side of the same goldens: tests/test_gpu_likelihoods.py."""
import math
import os

import numpy as np
import pytest
import torch

from gptorch_amd import likelihoods
from tests import _lik_cases as lc
from tests._util import ROOT, load_npz

T = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))


def data_term(lik, mu, v, y):
    """SVGP._data_term's generic route: one propagate_log per output column, the columns sharing the row's variance."""
    sd = torch.sqrt(v)
    return torch.stack([lik.propagate_log(torch.distributions.Normal(mu[:, j], sd), y[:, j]).reshape(()) for j in range(y.shape[1])]).sum()


@pytest.mark.parametrize("dy", [1, 3])
@pytest.mark.parametrize("H", lc.HS)
@pytest.mark.parametrize("g", range(len(lc.GROUPS)), ids=lc.GROUPS)
def test_torch_route_meets_the_goldens(g, H, dy):
    """value and autograd gradients of the torch route within 256 * 2^-53 * S of the same-rule expectation (S: the sum of the
    absolute values of the number's terms, stored beside it)."""
    c = lc.compose(g, lc.HS.index(H), 200, dy)
    lik = lc.make_likelihood(g, H)
    mu, v, y = T(c["mu"]).requires_grad_(True), T(c["v"]).requires_grad_(True), T(c["y"])
    val = data_term(lik, mu, v, y)
    params = [p for p in lik.parameters()]
    grads = torch.autograd.grad(val, [mu, v] + params)
    ratios = dict(val=lc.worst(val.item(), c["val"], c["val_S"]), dmu=lc.worst(grads[0].numpy(), c["dmu"], c["dmu_S"]),
                  dv=lc.worst(grads[1].numpy(), c["dv"], c["dv_S"]))
    if params:                                                # Student-t: d/d scale^2 from the gradient w.r.t. the raw parameter
        s = lik.scale.transform()
        ds2 = torch.autograd.grad((s * s).sum(), lik.scale)[0]
        ratios["dp"] = lc.worst((grads[2] / ds2).item(), c["dp"], c["dp_S"])
    print("%s H=%d dy=%d: worst |err| / (2^-53 S): %s" % (lc.GROUPS[g], H, dy, {k: round(r, 2) for k, r in ratios.items()}))
    for k, r in ratios.items():
        assert r < 256.0, (k, r)


def test_poisson_closed_form_equals_a_100_node_rule():
    """y mu - exp(mu + v/2) - lgamma(y + 1) against the 100-node rule of logp.  exp is entire and the rule integrates it to far
    below rounding at these v; what is left is the rounding of a 100-term fp64 sum whose terms are bounded by S = |y mu| +
    exp(mu + v/2) + lgamma(y + 1): 256 * 2^-53 * S as for the goldens."""
    g = lc.GROUPS.index("poisson")
    lik = lc.make_likelihood(g)
    for v0 in lc.VS:
        mu, y, v = T(lc.GOLD["mu"][g]), T(lc.GOLD["y"][g]), T(np.full(lc.E, v0))
        closed = y * mu - torch.exp(mu + 0.5 * v) - torch.lgamma(y + 1.0)
        S = (y * mu).abs() + torch.exp(mu + 0.5 * v) + torch.lgamma(y + 1.0).abs()
        by_rule = lc.rule(lambda f: lik.logp(f, y.unsqueeze(-1)), mu, v, 100)
        assert lik.propagate_log(torch.distributions.Normal(mu, torch.sqrt(v)), y).item() == pytest.approx(closed.sum().item(), rel=1e-15)
        assert lc.worst(by_rule.numpy(), closed.numpy(), S.numpy()) < 256.0


def _moments_by_rule(lik, mu, v, H):
    m = lc.rule(lik.conditional_mean, mu, v, H)
    return m, lc.rule(lambda f: lik.conditional_variance(f) + lik.conditional_mean(f) ** 2, mu, v, H) - m * m


def test_predictive_moments_closed_forms():
    """probit: p = Phi(mu / sqrt(1 + v)) against the 100-node rule, within twice what the 100-node rule differs from the
    200-node rule by (the reference's own error) plus rounding; Poisson and Student-t: the formulas of their moments, against
    the rule where it has converged the same way; the logit link's quadrature is a probability with variance p (1 - p)."""
    mu = T(np.linspace(-4.0, 4.0, 9)).repeat(len(lc.VS))
    v = T(np.repeat(lc.VS, 9))
    probit = likelihoods.Bernoulli()
    p, var = probit.predict_mean_variance(mu[:, None], v[:, None])
    assert p.shape == (36, 1) and var.shape == (36, 1)
    r100, r200 = lc.rule(probit.conditional_mean, mu, v, 100), lc.rule(probit.conditional_mean, mu, v, 200)
    own = (r100 - r200).abs()
    print("probit predictive mean: closed form vs 100 nodes %.2e, 100 vs 200 nodes %.2e" % ((p[:, 0] - r100).abs().max(), own.max()))
    assert bool(((p[:, 0] - r100).abs() <= 2.0 * own + 64 * lc.U).all())
    assert torch.equal(var, p * (1.0 - p))
    pois = likelihoods.Poisson()
    mu_p = 0.5 * mu
    m, s = pois.predict_mean_variance(mu_p[:, None], v[:, None])
    want_m = torch.exp(mu_p + 0.5 * v)
    want_s = want_m + (torch.exp(v) - 1.0) * want_m ** 2
    assert torch.allclose(m[:, 0], want_m, rtol=1e-15, atol=0) and torch.allclose(s[:, 0], want_s, rtol=1e-14, atol=0)
    m100, s100 = _moments_by_rule(pois, mu_p, v, 100)
    assert torch.allclose(m[:, 0], m100, rtol=1e-12, atol=0)            # exp is entire: the rule has converged to rounding
    assert torch.allclose(s[:, 0], s100, rtol=1e-10, atol=0)            # (E[y^2] - E[y]^2 cancels up to e^-v: 20 at v = 3)
    st = likelihoods.StudentT(df=4.0, scale=0.5)
    m, s = st.predict_mean_variance(mu[:, None], v[:, None])
    assert torch.equal(m[:, 0], mu) and torch.allclose(s[:, 0], v + 0.25 * 4.0 / 2.0, rtol=1e-15, atol=0)
    m20, s20 = likelihoods.Likelihood.predict_mean_variance(st, mu[:, None], v[:, None])    # polynomials of degree <= 2: exact
    assert torch.allclose(m20, m, rtol=0, atol=1e-14) and torch.allclose(s20, s, rtol=1e-13, atol=1e-14)
    logit = likelihoods.Bernoulli(link="logit")
    p, var = logit.predict_mean_variance(mu[:, None], v[:, None])
    assert bool(((p >= 0.0) & (p <= 1.0)).all()) and torch.equal(var, p * (1.0 - p))
    assert torch.allclose(p[:, 0], lc.rule(torch.sigmoid, mu, v, 20), rtol=1e-14, atol=0)
    assert torch.allclose(p[-9:, 0] + p[-9:, 0].flip(0), torch.ones(9, dtype=torch.float64), atol=1e-14)    # sigma(-f) = 1 - sigma(f)


# the truncation error of the default rule, H = 20 against H = 100, relative to max(1, |value|), over the golden grid
# (recorded in DESIGN 3.7d; measured by the test below, which prints what it finds)
TRUNCATION = {"probit": 2.5e-7, "logit": 2.3e-7, "student_t_default": 1.1e-4}   # all three at v = 3; <= 6e-7 at v = 1


@pytest.mark.parametrize("name", sorted(TRUNCATION))
def test_truncation_error_of_the_default_rule(name):
    """|rule_20 - rule_100| / max(1, |rule_100|) per entry of the golden grid stays within twice the recorded worst case, on the
    entries where the 100-node rule has itself converged: where it differs from the 200-node rule by at most 5 % of the
    recorded figure."""
    g = lc.GROUPS.index(name)
    lik = lc.make_likelihood(g)
    worst, kept = 0.0, 0
    for v0 in lc.VS:
        mu, y, v = T(lc.GOLD["mu"][g]), T(lc.GOLD["y"][g]), T(np.full(lc.E, v0))
        fn = lambda f: lik.logp(f, y.unsqueeze(-1)).detach()
        r20, r100, r200 = (lc.rule(fn, mu, v, H) for H in (20, 100, 200))
        scale = torch.clamp(r100.abs(), min=1.0)
        conv = ((r100 - r200).abs() / scale) <= 0.05 * TRUNCATION[name]
        kept += int(conv.sum())
        err = ((r20 - r100).abs() / scale)[conv]
        print("%s v = %g: H = 20 vs 100 %.3e (%d of %d entries converged at 100 nodes; 100 vs 200: %.1e)"
              % (name, v0, float(err.max()) if err.numel() else 0.0, int(conv.sum()), lc.E, float(((r100 - r200).abs() / scale).max())))
        if err.numel():
            worst = max(worst, float(err.max()))
    print("%s: worst %.3e (recorded %.1e)" % (name, worst, TRUNCATION[name]))
    assert kept >= 3 * lc.E                                   # (the check is not vacuous)
    assert worst <= 2.0 * TRUNCATION[name]
    assert worst >= 0.5 * TRUNCATION[name]                    # ... and the record is what the grid gives, not a loose ceiling


def test_interface_shapes_and_errors():
    mu, v, y = T(np.linspace(-1.0, 1.0, 6)), T(np.full(6, 0.3)), T([0.0, 1.0, 1.0, 0.0, 1.0, 0.0])
    qf = torch.distributions.Normal(mu, torch.sqrt(v))
    for lik in (likelihoods.Bernoulli(), likelihoods.Bernoulli(link="logit"), likelihoods.Poisson(), likelihoods.StudentT()):
        assert lik.num_gauss_hermite_points == 20
        out = lik.propagate_log(qf, y)
        assert out.dim() == 0 and bool(torch.isfinite(out))
        assert lik.logp(mu, y).shape == (6,)
        assert lik.conditional_mean(mu).shape == (6,) and lik.conditional_variance(mu).shape == (6,)
        m, s = lik.predict_mean_variance(mu[:, None], v[:, None])
        assert m.shape == (6, 1) and s.shape == (6, 1) and bool((s >= 0.0).all())
        with pytest.raises(TypeError, match="Expect Gaussian"):
            lik.propagate_log(torch.distributions.Laplace(mu, torch.sqrt(v)), y)
        with pytest.raises(ValueError, match="mismatch in size"):
            lik.propagate_log(qf, y[:5])
        with pytest.raises(NotImplementedError):
            lik.predict_mean_covariance(mu[:, None], torch.eye(6, dtype=torch.float64))
        for bad in (0, 65, 2.5, "20"):
            with pytest.raises(ValueError):
                lik.num_gauss_hermite_points = bad
        lik.num_gauss_hermite_points = 64
        assert lik.num_gauss_hermite_points == 64
    with pytest.raises(ValueError):
        likelihoods.Bernoulli(link="cloglog")
    with pytest.raises(ValueError):
        likelihoods.StudentT(df=2.0)
    st = likelihoods.StudentT(df=5.0, scale=0.7)
    assert isinstance(st.scale, likelihoods.Param) and st.scale.transform().item() == pytest.approx(0.7, rel=1e-14)
    assert [n for n, _ in st.named_parameters()] == ["scale"] and st.df == 5.0
    # a bare Likelihood has the rule but nothing to integrate
    with pytest.raises(NotImplementedError):
        likelihoods.Likelihood().propagate_log(qf, y)
    with pytest.raises(NotImplementedError):
        likelihoods.Likelihood().predict_mean_variance(mu[:, None], v[:, None])
    x1, w1 = likelihoods.gauss_hermite(20)
    x2, _ = likelihoods.gauss_hermite(20, "cpu")
    assert x1 is x2 and x1.dtype == torch.float64 and w1.sum().item() == pytest.approx(math.sqrt(math.pi), rel=1e-14)
    # a NaN, not an exception, for a negative variance (as the sqrt of the rule gives)
    neg =likelihoods.Likelihood._quadrature(likelihoods.Bernoulli(), mu, -v)[0]
    assert bool(torch.isnan(neg[:, 0]).all())


def test_gaussian_is_unchanged_on_the_reference_fixture():
    """likelihoods.Gaussian on the reference's sparse-GP fixture: logp, both predict_* and propagate_log give what their closed
    forms (likelihoods.py:92-144) give, and the class defines them itself (nothing is inherited from the new quadrature)."""
    f = load_npz("ref_sparse_gpr_fixtures.npz")
    y = T(f["y"])
    n = y.shape[0]
    mu = T(np.sin(np.arange(n, dtype=np.float64)))[:, None]
    var = T(0.1 + 0.05 * np.cos(np.arange(n, dtype=np.float64)) ** 2)[:, None]
    lik = likelihoods.Gaussian(variance=0.37)
    s2 = lik.variance.transform().item()
    assert s2 == pytest.approx(0.37, rel=1e-14)
    for name in ("logp", "predict_mean_variance", "predict_mean_covariance", "propagate_log"):
        assert name in likelihoods.Gaussian.__dict__
    want_logp = -0.5 * math.log(2.0 * math.pi * s2) - 0.5 * (y - mu) ** 2 / s2
    assert torch.allclose(lik.logp(mu, y), want_logp, rtol=1e-13, atol=1e-13)
    m, s = lik.predict_mean_variance(mu, var)
    assert torch.equal(m, mu) and torch.equal(s, var + lik.variance.transform())
    cov = torch.diag(var[:, 0]) + 0.01
    m, c = lik.predict_mean_covariance(mu, cov)
    assert torch.equal(m, mu) and torch.equal(c, cov + torch.eye(n, dtype=torch.float64) * lik.variance.transform())
    got = lik.propagate_log(torch.distributions.Normal(mu[:, 0], torch.sqrt(var[:, 0])), y[:, 0])
    want = -0.5 * (n * (math.log(2.0 * math.pi) + math.log(s2)) + (((y - mu) ** 2).sum().item() + (torch.sqrt(var) ** 2).sum().item()) / s2)
    assert got.shape == (1,) and got.item() == pytest.approx(want, rel=1e-14)


def test_native_entry_point_validates_before_any_launch():
    """gpn_lik_expect refuses bad arguments with -(argument index) on the host: nothing is launched, so this runs without a GPU
    (tests/test_gpu_likelihoods.py walks every argument)."""
    import ctypes
    from gptorch_amd import _native
    lib = _native.lib()
    one = (ctypes.c_double * 4)()
    p = ctypes.cast(one, ctypes.c_void_p)
    assert lib.gpn_lik_expect(None, 7, None, p, 1, p, p, 1, 10, 1, p, p, 20, p, 16, None, None, 1, None, None) == -2
    assert lib.gpn_lik_expect(None, _native.LIK_STUDENT_T, None, p, 1, p, p, 1, 10, 1, p, p, 20, p, 16, None, None, 1, None, None) == -3
    assert lib.gpn_lik_expect(None, _native.LIK_LOGIT, None, p, 1, p, p, 1, 10, 1, p, p, 65, p, 16, None, None, 1, None, None) == -13
    assert lib.gpn_lik_expect(None, _native.LIK_PROBIT, None, p, 1, p, p, 1, 257, 1, p, p, 20, p, 16, None, None, 1, None, None) == -15
    assert _native.LIK_ROWS_PER_GROUP == 256 and "GPN_LIK_ROWS_PER_GROUP 256" in open(os.path.join(ROOT, "include", "gpnative.h")).read()
