"""CPU suite: likelihoods.MultiClass (the robust-max multi-class likelihood) -- its torch route and autograd gradients against
the 40-digit goldens of tests/golden/make_multiclass_golden.py, the two-class rule against its closed form, the interface and
its errors, SVGP's construction with it (and without it: the same host draws as before), and the C ABI of its two entry points
(declared, bound, every argument validated before any launch).  The fused kernels' side: tests/test_gpu_multiclass.py.

Tolerance, per entry: max(16 e64, 64 * 2^-53 |golden|) with e64 the error of the oracle's plain-fp64 statement (the rule of
tests/test_gpu_laplace.py for pointwise quantities).  A sum of n row values gets the rows' tolerances plus n * 2^-53 sum |terms|
(n: the depth of a sequential sum, an upper bound for torch's)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from gptorch_amd import _native, kernels, likelihoods
from gptorch_amd.models import SVGP, EPGP, LaplaceGP
from tests import _multiclass_oracle as mo
from tests._util import ROOT, load_npz

GOLD = load_npz("multiclass_cases.npz")
META = json.loads(str(GOLD["meta"]))
U = 2.0 ** -53
T = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))


def entry_tol(C, H, key):
    gold, e64 = GOLD["C%d_H%d_%s" % (C, H, key)], GOLD["C%d_H%d_%s_e64" % (C, H, key)]
    return gold, np.maximum(16.0 * e64, 64.0 * U * np.abs(gold))


def make_lik(C, H):
    lik = likelihoods.MultiClass(C, epsilon=META["eps"])
    lik.num_gauss_hermite_points = H
    return lik


def test_golden_inputs_are_the_oracles_points():
    for C in mo.CLASSES:
        mu, v, lab = mo.points(C)
        assert np.array_equal(mu, GOLD["C%d_mu" % C]) and np.array_equal(v, GOLD["C%d_v" % C]) and np.array_equal(lab, GOLD["C%d_label" % C])
        gaps = (mu[np.arange(len(v)), lab.astype(int)][:, None] - mu) / np.sqrt(v)[:, None]
        assert gaps.max() > 39.0 and gaps.min() < -39.0 and set(v) == set(mo.POINT_V)
        assert np.any(np.sum(gaps == 0.0, 1) == C)                       # a row of ties


@pytest.mark.parametrize("H", mo.HS)
@pytest.mark.parametrize("C", mo.CLASSES)
def test_torch_route_and_autograd_meet_the_goldens(C, H):
    mu, v, lab = T(GOLD["C%d_mu" % C]).requires_grad_(True), T(GOLD["C%d_v" % C]).requires_grad_(True), T(GOLD["C%d_label" % C])
    lik = make_lik(C, H)
    val = lik.variational_expectation(mu, v, lab)
    g_mean, g_var = torch.autograd.grad(val, [mu, v])
    for key, got in (("gm", g_mean), ("gv", g_var)):
        gold, tol = entry_tol(C, H, key)
        err = np.abs(got.numpy() - gold)
        print("C=%d H=%d %s: worst err / tol %.3f" % (C, H, key, np.max(err / np.maximum(tol, 1e-300))))
        assert np.all(err <= tol), (key, int(np.argmax(err / np.maximum(tol, 1e-300))))
    gold, tol = entry_tol(C, H, "val")
    bound = float(np.sum(tol) + len(gold) * U * np.sum(np.abs(gold)))
    assert abs(val.item() - float(np.sum(gold.astype(np.longdouble)))) <= bound
    p, var = lik.predict_mean_variance(mu.detach(), v.detach())
    gold, tol = entry_tol(C, H, "probs")
    assert np.all(np.abs(p.numpy() - gold) <= tol)
    assert torch.equal(var, p * (1.0 - p))
    # the variance may come as [n], [n, 1] or expanded over the columns (what SVGP's predict_f returns)
    assert torch.equal(lik.predict_mean_variance(mu.detach(), v.detach()[:, None].expand(-1, C))[0], p)


def test_far_on_the_wrong_side_everything_is_exactly_zero():
    """the labelled latent 60 standard deviations below another (Phi(-60 + 7.7) = 1e-596 at the rule's outermost node): P and
    every gradient underflow to 0, nothing is NaN."""
    lik = make_lik(3, 20)
    mu, v = T([[0.0, 60.0, 1.0]]).requires_grad_(True), T([1.0]).requires_grad_(True)
    val = lik.variational_expectation(mu, v, T([0.0]))
    g_mean, g_var = torch.autograd.grad(val, [mu, v])
    assert val.item() == pytest.approx(np.log(META["eps"] / 2.0), rel=1e-15)
    assert torch.equal(g_mean, torch.zeros(1, 3, dtype=torch.float64)) and g_var.item() == 0.0


def test_two_classes_equal_the_probit_closed_form():
    """C = 2, H = 64: P = Phi((mu_y - mu_o) / sqrt(2 v)) up to the accuracy of the 64-node rule, which the generator measured in
    40 digits on this grid of gaps (META: far below fp64 rounding -- the integrand is smooth at v = 1); the bound is that plus
    16 * 2^-53 for the fp64 evaluation of a number <= 1."""
    rule = META["c2_h64_rule_accuracy"]
    assert rule < U
    lik = make_lik(2, 64)
    gaps = np.arange(-6.0, 6.01, 0.5)
    v = 0.7
    mu = T(np.stack([0.2 + np.sqrt(v) * gaps, np.full(gaps.size, 0.2)], 1))
    p, _ = lik.predict_mean_variance(mu, T(np.full(gaps.size, v)))
    eps = META["eps"]
    P = (p[:, 0] - eps) / (1.0 - 2.0 * eps)                                  # p = (1 - eps) P + eps (1 - P)
    want = torch.special.ndtr(T(gaps) / np.sqrt(2.0))
    err = float((P - want).abs().max())
    print("C = 2, H = 64: |P - Phi| %.2e (rule %.2e)" % (err, rule))
    assert err <= rule + 16.0 * U
    assert float((p.sum(1) - 1.0).abs().max()) <= 4.0 * U                    # the two-class rule is symmetric


def test_logp_is_the_pointwise_definition():
    lik = likelihoods.MultiClass(3, epsilon=0.1)
    F = T([[0.0, 1.0, 0.5], [2.0, 1.0, 0.0], [0.0, -1.0, 3.0]])
    lp = lik.logp(F, T([[1.0], [1.0], [2.0]]))
    assert lp.shape == (3, 1)
    assert np.allclose(lp[:, 0].numpy(), [np.log(0.9), np.log(0.05), np.log(0.9)], rtol=1e-15, atol=0)
    assert lik.logp(F, T([1.0, 1.0, 2.0])).shape == (3,)


def test_constructor_and_interface_errors():
    for bad in (1, 0, -3, 2.5):
        with pytest.raises(ValueError):
            likelihoods.MultiClass(bad)
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            likelihoods.MultiClass(3, epsilon=bad)
    lik = likelihoods.MultiClass(4)
    assert lik.num_latent == 4 and lik.epsilon == 1e-3 and isinstance(lik, likelihoods._NonGaussian)
    with pytest.raises(NotImplementedError, match="variational_expectation"):
        lik.propagate_log(torch.distributions.Normal(torch.zeros(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64)), torch.zeros(3))
    with pytest.raises(NotImplementedError):
        lik.predict_mean_covariance(torch.zeros(3, 4), torch.eye(3))
    with pytest.raises(ValueError):
        lik.variational_expectation(torch.zeros(5, 3, dtype=torch.float64), torch.ones(5, dtype=torch.float64), torch.zeros(5))
    with pytest.raises(ValueError):
        lik.variational_expectation(torch.zeros(5, 4, dtype=torch.float64), torch.ones(4, dtype=torch.float64), torch.zeros(5))
    with pytest.raises(ValueError):
        lik.variational_expectation(torch.zeros(5, 4, dtype=torch.float64), torch.ones(5, dtype=torch.float64), torch.zeros(6))


def _data(n=60, C=3, seed=5):
    r = np.random.RandomState(seed)
    x = r.randn(n, 2)
    return x, (np.arange(n) % C).astype(np.float64)[:, None]


def test_svgp_carries_one_latent_column_per_class():
    x, y = _data()
    np.random.seed(3)
    m = SVGP(x, y, kernels.Rbf(2), inducing_points=x[:12].copy(), likelihood=likelihoods.MultiClass(3))
    assert m.induced_output_mean.shape == (12, 3) and m.Y.shape == (60, 1)
    assert tuple(m.induced_output_chol_cov.shape) == (12, 12)
    assert bool(torch.isfinite(m.induced_output_mean).all())


def test_svgp_checks_the_labels_once_at_construction():
    x, y = _data()
    for bad in (y + 0.5, y - 1.0, np.where(y == 2.0, 3.0, y), np.concatenate([y, y], 1)):
        with pytest.raises(ValueError):
            SVGP(x, bad, kernels.Rbf(2), inducing_points=x[:12].copy(), likelihood=likelihoods.MultiClass(3))


def test_other_likelihoods_consume_the_same_host_draws():
    """SVGP's constructor makes exactly ONE np.random.permutation(N) draw when the inducing points are given -- with Bernoulli as
    before this feature, and with MultiClass too: the next draw of the stream says so."""
    x, y = _data()
    for lik, yy in ((likelihoods.Bernoulli(), (y > 0).astype(np.float64)), (likelihoods.MultiClass(3), y)):
        np.random.seed(123)
        m = SVGP(x, yy, kernels.Rbf(2), inducing_points=x[:12].copy(), likelihood=lik)
        got = np.random.rand()
        np.random.seed(123)
        np.random.permutation(60)
        assert got == np.random.rand()
        assert m.induced_output_mean.shape[1] == (3 if isinstance(lik, likelihoods.MultiClass) else 1)


def test_exact_gp_classifiers_still_refuse_it():
    x, y = _data()
    for cls in (LaplaceGP, EPGP):
        with pytest.raises((TypeError, ValueError, NotImplementedError)):
            cls(x, y, kernels.Rbf(2), likelihood=likelihoods.MultiClass(3))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_native_binds_the_entry_points():
    text = open(os.path.join(ROOT, "include", "gpnative.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name, nargs in (("gpn_lik_expect_robustmax", 17), ("gpn_lik_robustmax_probs", 12)):
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == nargs == len(_native.SIGNATURES[name][1])
        assert not re.search(r"\bint\s+kind\b", decl.group(1))               # not a kernel-kind-dispatched entry
        assert hasattr(lib, name)
    assert "#define GPN_ROBUSTMAX_ROWS_PER_GROUP %d" % _native.ROBUSTMAX_ROWS_PER_GROUP in text


def test_argument_validation_without_launch():
    """-(argument position) before any HIP call: every pointer is NULL or a host address that is never followed."""
    lib = _native.lib()
    p = ctypes.cast((ctypes.c_double * 4)(), ctypes.c_void_p)
    ok = dict(f_mean=p, ldf=3, f_var=p, labels=p, rows=10, C=3, eps=1e-3, nodes=p, weights=p, H=20, work=p, work_bytes=24, value=None,
              g_mean=None, ldg=3, g_var=None)

    def expect(**kw):
        a = dict(ok, **kw)
        return lib.gpn_lik_expect_robustmax(None, a["f_mean"], a["ldf"], a["f_var"], a["labels"], a["rows"], a["C"], a["eps"], a["nodes"],
                                            a["weights"], a["H"], a["work"], a["work_bytes"], a["value"], a["g_mean"], a["ldg"], a["g_var"])
    assert expect(f_mean=None) == -2
    assert expect(ldf=2) == -3
    assert expect(f_var=None) == -4
    assert expect(labels=None) == -5
    assert expect(rows=0) == -6 and expect(rows=-1) == -6
    assert expect(C=1) == -7 and expect(C=0) == -7
    assert expect(eps=0.0) == -8 and expect(eps=1.0) == -8 and expect(eps=float("nan")) == -8
    assert expect(nodes=None) == -9
    assert expect(weights=None) == -10
    assert expect(H=0) == -11 and expect(H=65) == -11
    assert expect(work=None) == -12
    assert expect(work_bytes=16) == -13 and expect(rows=13, work_bytes=24) == -13
    assert expect(g_mean=p, ldg=2) == -16
    assert expect(rows=1 << 34, work_bytes=1 << 40) == -102                  # GPN_E_UNSUPPORTED: more workgroups than a grid holds

    okp = dict(f_mean=p, ldf=3, f_var=p, rows=10, C=3, eps=1e-3, nodes=p, weights=p, H=20, probs=p, ldp=3)

    def probs(**kw):
        a = dict(okp, **kw)
        return lib.gpn_lik_robustmax_probs(None, a["f_mean"], a["ldf"], a["f_var"], a["rows"], a["C"], a["eps"], a["nodes"], a["weights"],
                                           a["H"], a["probs"], a["ldp"])
    assert probs(f_mean=None) == -2
    assert probs(ldf=2) == -3
    assert probs(f_var=None) == -4
    assert probs(rows=0) == -5
    assert probs(C=1) == -6
    assert probs(eps=0.0) == -7 and probs(eps=1.0) == -7
    assert probs(nodes=None) == -8
    assert probs(weights=None) == -9
    assert probs(H=0) == -10 and probs(H=65) == -10
    assert probs(probs=None) == -11
    assert probs(ldp=2) == -12
    assert lib.gpn_last_hip_error() == b""
