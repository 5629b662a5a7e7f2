"""EPGP, the part that needs no GPU: the host oracle's closed-form gradient against central differences of its own converged
evidence, its parallel fixed point against sequential EP (R&W Algorithm 3.5), its rearranged evidence against the textbook formula,
the construction errors, the lock-step grouping, and the argument validation of gpn_ep_sites (no launch)."""
import numpy as np
import pytest

from gptorch_amd import _native, kernels, likelihoods, rng
from gptorch_amd.models import EPGP, LaplaceGP, _lockstep
from tests import _ep_oracle as eo


def problem(n, d, seed, lik="probit"):
    x = rng.normal(seed, (n, d))
    g = np.sin(1.3 * x[:, 0]) + 0.5 * x[:, 1]
    y = (rng.uniform(seed + 1, n) < 1.0 / (1.0 + np.exp(-2.0 * g))).astype(np.float64)
    return x, y


@pytest.mark.parametrize("lik", ["probit", "logit"])
def test_oracle_gradient_matches_central_differences(lik):
    """d loss/d(log variance, log length_scales, mean) in closed form (no implicit term: R&W eq. 5.27) against central differences
    of the fp64 evidence swept until the change stops shrinking.  Step h = 1e-5, bound 1e-7 max(1, |g|): truncation
    h^2 / 6 |f'''| = 1.7e-11 |f'''|; rounding 2 eps |loss| / (2 h) with the converged evidence good to a few 1e-14 |loss| ~ 1e-12,
    so ~ 1e-7 at worst and 1e-9 as observed."""
    n, d, h = 120, 2, 1e-5
    x, y = problem(n, d, 7)
    theta0 = np.array([np.log(1.3), np.log(0.9), np.log(1.4), 0.25])          # log variance, log ell (ARD), mean

    def oracle(theta):
        return eo.EPOracle(x, y, "Matern52", lik, np.exp(theta[0]), np.exp(theta[1:3]), ARD=True, mean=theta[3]).search(until_stall=True)

    got = np.concatenate([np.asarray(g_, dtype=np.float64).ravel() for g_ in oracle(theta0).loss_grads()])
    for i in range(theta0.size):
        e = np.zeros_like(theta0)
        e[i] = h
        fd = float((oracle(theta0 + e).loss() - oracle(theta0 - e).loss()) / (2 * h))
        print("%s d/dtheta[%d]: closed %.10f central %.10f" % (lik, i, got[i], fd))
        assert abs(got[i] - fd) <= 1e-7 * max(1.0, abs(fd))


def test_parallel_fixed_point_is_the_sequential_one():
    """damped parallel sweeps and R&W Algorithm 3.5 (one site at a time, rank-one updates) reach the same sites, evidence and
    marginals: 1e-8, relative to max(1, |value|)."""
    n = 60
    x, y = problem(n, 2, 21)
    par = eo.EPOracle(x, y, "Rbf", "probit", 1.7, [0.9], mean=0.2).search(until_stall=True)
    seq = eo.EPOracle(x, y, "Rbf", "probit", 1.7, [0.9], mean=0.2)
    tau, nu, mu, sigma2 = seq.sequential()
    seq.settle(tau, nu)
    for name, a, b in (("tau", par.tau, tau), ("nu", par.nu, nu), ("mu", par.mu, mu), ("sigma2", par.sigma2, sigma2),
                       ("evidence", par.log_evidence(), seq.log_evidence())):
        err = float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1.0, np.abs(np.asarray(b)))))
        print("parallel vs sequential %-8s %.2e" % (name, err))
        assert err <= 1e-8, name


def test_rearranged_evidence_equals_the_textbook_formula():
    """sum e_i + 1/2 w^T K a - sum log L_ii against sum log Z~_i + log N(mu~ | m, K + Sigma~) as written, on a case whose site
    precisions all exceed 1e-3.  The textbook form divides by tau: the condition number of K + Sigma~ is at most
    (n variance + 1 / tau_min) tau_max < 2e3 here, times 2^-53 and the size of the quadratic terms (< 1e3): 1e-9 relative to
    max(1, |log Z|) is two orders above that."""
    n = 120
    x, y = problem(n, 2, 31)
    o = eo.EPOracle(x, y, "Rbf", "probit", 1.7, [0.9], mean=0.3).search()
    assert o.tau.min() > 1e-3 and o.tau.max() < 1.0
    a, b = float(o.log_evidence()), float(o.log_evidence_direct())
    print("evidence rearranged %.12f textbook %.12f (min tau %.3g)" % (a, b, o.tau.min()))
    assert abs(a - b) <= 1e-9 * max(1.0, abs(b))


def test_construction_errors_name_the_alternative():
    x, y = rng.normal(1, (20, 2)), (rng.uniform(2, 20) < 0.5).astype(np.float64).reshape(20, 1)
    rbf = kernels.Rbf(2)
    with pytest.raises(NotImplementedError, match="SVGP"):
        EPGP(x, y, kernels.Rbf(2) + kernels.Matern52(2), likelihoods.Bernoulli())
    with pytest.raises(NotImplementedError, match="SVGP"):
        EPGP(x, y, kernels.Linear(2), likelihoods.Bernoulli())
    with pytest.raises(NotImplementedError, match="log-concave"):
        EPGP(x, y, rbf, likelihoods.StudentT())
    with pytest.raises(ValueError, match="GPR"):
        EPGP(x, y, rbf, likelihoods.Gaussian())
    with pytest.raises(NotImplementedError, match="LaplaceGP takes Poisson"):
        EPGP(x, y, rbf, likelihoods.Poisson())

    class Mine(likelihoods.Bernoulli):
        pass

    with pytest.raises(NotImplementedError, match="Bernoulli"):
        EPGP(x, y, rbf, Mine())
    with pytest.raises(ValueError, match=r"\[N, 1\]"):
        EPGP(x, np.repeat(y, 2, 1), rbf, likelihoods.Bernoulli())
    for lik in (likelihoods.Bernoulli("probit"), likelihoods.Bernoulli("logit")):
        m = EPGP(x, y, kernels.Matern52(2, ARD=True), lik)
        assert m.ep_stats == {"sweeps": 0, "stalled": False} and m.warm_start
        assert (m.ep_tol, m.max_sweeps, m.damping) == (1e-10, 200, 0.8)
        with pytest.raises(NotImplementedError):
            m.likelihood.predict_mean_covariance(None, None)           # what predict_y(diag=False) and predict_y_samples run into


def test_lock_step_grouping_leaves_ep_models_alone():
    x, y = rng.normal(1, (30, 2)), (rng.uniform(2, 30) < 0.5).astype(np.float64).reshape(30, 1)
    ms = [EPGP(x, y, kernels.Rbf(2), likelihoods.Bernoulli("probit")) for _ in range(3)]
    assert _lockstep._laplace_groups(ms) == []
    # ... and not merely because these models live on the host: the grouping asks for LaplaceGP's own log_likelihood
    assert not any(isinstance(m, LaplaceGP) for m in ms)
    assert EPGP.log_likelihood is not LaplaceGP.log_likelihood and EPGP._predict is LaplaceGP._predict


def test_argument_validation_without_launch():
    """gpn_ep_sites rejects bad arguments with -(argument index) / GPN_E_* before any HIP call (null pointers throughout)."""
    lib = _native.lib()
    null = None

    def call(kind=_native.LIK_PROBIT, n=4, damping=0.8, H=0, moments_only=0):
        # (stream, kind, n, y, m, mu, sigma2, tau, nu, damping, nodes, weights, H, moments_only, work, work_bytes, tau_out, nu_out,
        #  lz, mu_hat, s2_hat, stats)
        return lib.gpn_ep_sites(null, kind, n, null, null, null, null, null, null, damping, null, null, H, moments_only, null, 0,
                                null, null, null, null, null, null)

    assert call(kind=7) == -2
    assert call(kind=_native.LIK_POISSON) == -102 and call(kind=_native.LIK_STUDENT_T) == -102
    assert call(n=0) == -3
    assert call() == -4
    assert lib.gpn_ep_sites_work_bytes(0) == 0 and lib.gpn_ep_sites_work_bytes(256) == 6 * 8 and lib.gpn_ep_sites_work_bytes(257) == 2 * 6 * 8
