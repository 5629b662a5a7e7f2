"""LaplaceGP, the part that needs no GPU: the host oracle's closed-form gradient against central differences of its own
long-double value, Likelihood.logp_derivatives against the 40-digit goldens and against autograd, the construction errors, and
the argument validation of every new entry point (no launch)."""
import numpy as np
import pytest
import torch

from gptorch_amd import _native, kernels, likelihoods, rng
from gptorch_amd.models import LaplaceGP
from tests import _laplace_oracle as lo
from tests import _xref as xr
from tests._util import load_npz

GOLD = load_npz("laplace_cases.npz")
U = 2.0 ** -53


def pointwise_tol(lik, name):
    """the issue's rule for the pointwise quantities: max(16 e64, 64 * 2^-53 |golden|), per entry."""
    return np.maximum(16.0 * GOLD["pw_%s_%s_e64" % (lik, name)], 64.0 * U * np.abs(GOLD["pw_%s_%s" % (lik, name)]))


def _likelihood(lik):
    return likelihoods.Poisson() if lik == "poisson" else likelihoods.Bernoulli(lik)


@pytest.mark.parametrize("lik", ["probit", "logit", "poisson"])
def test_oracle_gradient_matches_central_differences(lik):
    """d loss/d(log variance, log length_scales, mean) in closed form against central differences of the converged long-double
    value.  Step h = 1e-4 in every parameter: truncation h^2 / 6 |f'''| = 1.7e-9 |f'''|, rounding 2 eps |loss| / h ~ 1e-13 with
    eps = 2^-64 and a search iterated until it stalls.  The bound 1e-6 max(1, |g|) leaves room for |f'''| up to 600."""
    n, d, h = 40, 2, 1e-4
    x = rng.normal(7, (n, d))
    g = np.sin(1.3 * x[:, 0]) + 0.5 * x[:, 1]
    u = rng.uniform(8, n)
    y = np.floor(-np.log(u) * np.exp(0.8 + g)) if lik == "poisson" else (u < 1.0 / (1.0 + np.exp(-2.0 * g))).astype(np.float64)
    theta0 = np.array([np.log(1.3), np.log(0.9), np.log(1.4), 0.25])          # log variance, log ell (ARD), mean

    def oracle(theta):
        return lo.LaplaceOracle(x, y, "Matern52", lik, np.exp(lo.LD(theta[0])), np.exp(np.asarray(theta[1:3], dtype=lo.LD)), ARD=True,
                                mean=lo.LD(theta[3]), dtype=lo.LD).search(until_stall=True)

    got = np.concatenate([np.asarray(g_, dtype=np.float64).ravel() for g_ in oracle(theta0).loss_grads()])
    for i in range(theta0.size):
        e = np.zeros_like(theta0)
        e[i] = h
        fd = float((oracle(theta0 + e).loss() - oracle(theta0 - e).loss()) / (2 * lo.LD(h)))
        print("%s d/dtheta[%d]: closed %.10f central %.10f" % (lik, i, got[i], fd))
        assert abs(got[i] - fd) <= 1e-6 * max(1.0, abs(fd))


@pytest.mark.parametrize("lik", ["probit", "logit", "poisson"])
def test_logp_derivatives_match_the_goldens(lik):
    F, Y = torch.tensor(GOLD["pw_%s_f" % lik]), torch.tensor(GOLD["pw_%s_y" % lik])
    got = _likelihood(lik).logp_derivatives(F, Y)
    for name, g in zip(("lp", "d1", "W", "d3"), got):
        err = np.abs(g.numpy() - GOLD["pw_%s_%s" % (lik, name)])
        tol = pointwise_tol(lik, name)
        print("%s %s: worst err / tol %.3f" % (lik, name, np.max(err / np.maximum(tol, 1e-300))))
        assert np.all(err <= tol), (lik, name, np.argmax(err / np.maximum(tol, 1e-300)))


@pytest.mark.parametrize("lik", ["probit", "logit", "poisson"])
def test_logp_derivatives_match_autograd(lik):
    """d1 against autograd of logp, W and d3 against autograd of the closed forms one order below: two fp64 evaluations of one
    function.  On |f| <= 5 the probit forms cancel by at most z^2 = 25 in z + r and again in (z + r)(z + 2 r) - 1: a condition
    number below 1e3, times a few ulps per operation (64 * 2^-53), gives 1e-11 relative to max(1, |value|).  (An even number of
    grid points: the logit forms are written in |f|, whose autograd derivative at exactly f = 0 is the subgradient 0.)"""
    L = _likelihood(lik)
    f = torch.linspace(-5.0, 5.0, 40, dtype=torch.float64).repeat(2).requires_grad_(True)
    y = torch.cat([torch.zeros(40, dtype=torch.float64), torch.ones(40, dtype=torch.float64)]) if lik != "poisson" \
        else torch.cat([torch.full((40,), 2.0, dtype=torch.float64), torch.full((40,), 30.0, dtype=torch.float64)])
    lp, d1, W, d3 = L.logp_derivatives(f, y)
    assert torch.equal(lp.detach(), L.logp(f, y).detach()) or xr.rel_err(lp, L.logp(f, y)) <= 64 * U
    for name, closed, lower, sign in (("d1", d1, L.logp(f, y), 1.0), ("W", W, d1, -1.0), ("d3", d3, W, -1.0)):
        auto = sign * torch.autograd.grad(lower.sum(), f, retain_graph=True)[0]
        err = float(((closed - auto).abs() / torch.clamp(auto.abs(), min=1.0)).max().detach())
        print("%s %s vs autograd: %.2e" % (lik, name, err))
        assert err <= 1e-11


def test_base_likelihood_has_no_derivatives():
    with pytest.raises(NotImplementedError):
        likelihoods.StudentT().logp_derivatives(torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64))
    with pytest.raises(NotImplementedError):
        likelihoods.Gaussian().logp_derivatives(torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64))


def test_construction_errors_name_the_alternative():
    x, y = rng.normal(1, (20, 2)), (rng.uniform(2, 20) < 0.5).astype(np.float64).reshape(20, 1)
    rbf = kernels.Rbf(2)
    with pytest.raises(NotImplementedError, match="SVGP"):
        LaplaceGP(x, y, kernels.Rbf(2) + kernels.Matern52(2), likelihoods.Bernoulli())
    with pytest.raises(NotImplementedError, match="SVGP"):
        LaplaceGP(x, y, kernels.Linear(2), likelihoods.Bernoulli())
    with pytest.raises(NotImplementedError, match="SVGP"):
        LaplaceGP(x, y, kernels.White(2), likelihoods.Bernoulli())
    with pytest.raises(NotImplementedError, match="log-concave"):
        LaplaceGP(x, y, rbf, likelihoods.StudentT())
    with pytest.raises(ValueError, match="GPR"):
        LaplaceGP(x, y, rbf, likelihoods.Gaussian())
    with pytest.raises(ValueError, match=r"\[N, 1\]"):
        LaplaceGP(x, np.repeat(y, 2, 1), rbf, likelihoods.Bernoulli())
    for lik in (likelihoods.Bernoulli("probit"), likelihoods.Bernoulli("logit"), likelihoods.Poisson()):
        m = LaplaceGP(x, y, kernels.Matern52(2, ARD=True), lik)
        assert m.newton_stats == {"steps": 0, "halvings": 0} and m.warm_start


def test_argument_validation_without_launch():
    """every new entry point rejects bad arguments with -(argument index) / GPN_E_* before any HIP call (null pointers throughout,
    as tests/test_abi.py does for its neighbours)."""
    lib = _native.lib()
    null = None
    # gpn_lik_derivs(stream, kind, f, y, n, work, work_bytes, value, d1, w, d3)
    assert lib.gpn_lik_derivs(null, 7, null, null, 4, null, 0, null, null, null, null) == -2
    assert lib.gpn_lik_derivs(null, _native.LIK_STUDENT_T, null, null, 4, null, 0, null, null, null, null) == -102
    assert lib.gpn_lik_derivs(null, _native.LIK_PROBIT, null, null, 4, null, 0, null, null, null, null) == -3
    assert lib.gpn_lik_derivs_work_bytes(1) == 8 and lib.gpn_lik_derivs_work_bytes(257) == 16 and lib.gpn_lik_derivs_work_bytes(0) == 0
    # gpn_laplace_system(stream, kind, X, n, d, variance, length_scales, nls, s, A, lda)
    assert lib.gpn_laplace_system(null, 9, null, 4, 2, null, null, 1, null, null, 128) == -2
    assert lib.gpn_laplace_system(null, 0, null, 4, 2, null, null, 1, null, null, 128) == -3
    # gpn_laplace_matvec(stream, kind, X, n, d, variance, length_scales, nls, v, work, out)
    assert lib.gpn_laplace_matvec(null, -1, null, 4, 2, null, null, 1, null, null, null) == -2
    assert lib.gpn_laplace_matvec(null, 1, null, 4, 0, null, null, 1, null, null, null) == -3
    assert lib.gpn_laplace_rows_work_bytes(65) == 2 * 2 * 64 * 8 and lib.gpn_laplace_rows_work_bytes(0) == 0
    # gpn_laplace_diag(stream, kind, X, n, d, variance, length_scales, nls, s, Binv, ldb, work, sigma)
    assert lib.gpn_laplace_diag(null, 6, null, 4, 2, null, null, 1, null, null, 4, null, null) == -2
    assert lib.gpn_laplace_diag(null, 0, null, 4, 2, null, null, 1, null, null, 4, null, null) == -3
    # gpn_laplace_grad(stream, kind, X, n, d, variance, length_scales, nls, s, Binv, ldb, a, u, d1, work, out)
    assert lib.gpn_laplace_grad(null, 6, null, 4, 2, null, null, 1, null, null, 4, null, null, null, null, null) == -2
    assert lib.gpn_laplace_grad(null, 0, null, 4, 2, null, null, 1, null, null, 4, null, null, null, null, null) == -3
    assert lib.gpn_laplace_grad_work_bytes(128, 3) == 3 * 4 * 8 and lib.gpn_laplace_grad_work_bytes(129, 1) == 6 * 2 * 8
    # gpn_backsub(stream, A, lda, winv, n, dy, work, out, ldo)
    assert lib.gpn_backsub(null, null, 128, null, 4, 1, null, null, 4) == -2
    assert lib.gpn_backsub_work_bytes(300, 1) == 2 * 384 * 8 and lib.gpn_backsub_work_bytes(300, 0) == 0
