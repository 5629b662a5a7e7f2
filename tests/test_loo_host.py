"""The leave-one-out objective of GPR, the part that needs no GPU: the host oracle's closed form against real refits and against
central differences of its own long-double value, the argument validation of every gpn_loo_* entry point (no launch), and the
`objective` keyword."""
import json

import numpy as np
import pytest

from gptorch_amd import _native, kernels, rng
from gptorch_amd.models import GPR
from tests import _loo_oracle as lo
from tests import _xref as xr
from tests._util import load_npz
from tests.golden import make_loo_golden as maker

GOLD = load_npz("loo_cases.npz")
CASES = {c["name"]: c for c in json.loads(str(GOLD["meta"]))["cases"]}
EPS = 2.0 ** -52


def test_closed_form_equals_refits():
    """Every one of the 300 held-out means and variances of the Rbf case, closed form in long double against the stored long-double
    refits (each a fresh factorisation of the other 299 points, rounded to fp64 when stored: 2^-53 by itself), and three refits
    done again here against the stored ones.  Bound: 2^-52 relative to max(1, |value|), per quantity.
    Observed when the golden was made: 9.2e-18 between the two long-double statements before the rounding to fp64, i.e. the
    stored-value comparison sits at the fp64 rounding of the goldens, 1.1e-16 at most."""
    case = CASES["rbf_300x2"]
    ref, _ = maker.build(case)
    mean, var = ref.loo_predict()
    for name, got, want in (("mean", mean[:, 0], GOLD["rbf_300x2__refit_mean"][:, 0]), ("var", var[:, 0], GOLD["rbf_300x2__refit_var"])):
        err = xr.rel_err(got, want)
        print("closed form vs stored refits, %s: %.2e (bound %.2e)" % (name, err, EPS))
        assert err <= EPS
    for i in (0, 137, 299):
        m, v = ref.refit(i)
        assert abs(float(m[0]) - GOLD["rbf_300x2__refit_mean"][i, 0]) <= EPS * max(1.0, abs(float(m[0])))
        assert abs(float(v) - GOLD["rbf_300x2__refit_var"][i]) <= EPS * max(1.0, abs(float(v)))
        # and directly, both sides in long double
        assert abs(m[0] - mean[i, 0]) <= EPS * max(1.0, abs(float(m[0]))) and abs(v - var[i, 0]) <= EPS * max(1.0, abs(float(v)))


def test_oracle_value_is_the_sum_of_the_refit_densities():
    """L_LOO of the oracle = sum_i log N(y_i | refit mean_i, refit variance_i) with the stored refits: the closed-form VALUE, not only
    its means and variances.  300 terms of magnitude <= 4, each good to the fp64 rounding of the stored mean and variance
    (2^-53, amplified by (y - mu) / sigma^2 <= 30): bound 300 * 64 * 2^-53 = 2.1e-12 absolute on |L_LOO| ~ 116."""
    case = CASES["rbf_300x2"]
    _, y = maker.case_inputs(case)
    mu, s2 = GOLD["rbf_300x2__refit_mean"][:, 0].astype(lo.LD), GOLD["rbf_300x2__refit_var"].astype(lo.LD)
    total = np.sum(-0.5 * np.log(2 * lo.LD(np.pi) * s2) - 0.5 * (y[:, 0].astype(lo.LD) - mu) ** 2 / s2)
    print("sum of refit log densities %.12f, golden -loss %.12f" % (float(total), -case["loss"]))
    assert abs(float(total) + case["loss"]) <= 300 * 64 * 2.0 ** -53


def test_oracle_gradient_matches_central_differences():
    """d(-L_LOO)/d(log variance, log ell (ARD), log noise, mean) in closed form against central differences of the long-double
    value.  Step h = 1e-4: truncation h^2 / 6 |f'''| = 1.7e-9 |f'''|, rounding 2 eps |loss| / h ~ 1e-13 with eps = 2^-64.  The bound
    1e-6 max(1, |g|) leaves room for |f'''| up to 600 (tests/test_laplace_host.py uses the same step and bound)."""
    n, d, dy, h = 40, 3, 2, 1e-4
    x, y = rng.make_regression(n, d, dy, seed=41)
    theta0 = np.array([np.log(1.3), np.log(0.9), np.log(1.4), np.log(0.7), np.log(0.04), 0.25, -0.1])

    def oracle(theta):
        t = np.asarray(theta, dtype=lo.LD)
        return lo.LooRef(x, y, "Matern52", np.exp(t[0]), np.exp(t[1:4]), np.exp(t[4]), ARD=True, mean=t[5:7])

    got = np.concatenate([np.asarray(g, dtype=np.float64).ravel() for g in oracle(theta0).loss_grads()])
    for i in range(theta0.size):
        e = np.zeros_like(theta0)
        e[i] = h
        fd = float((oracle(theta0 + e).loss() - oracle(theta0 - e).loss()) / (2 * lo.LD(h)))
        print("d/dtheta[%d]: closed %.10f central %.10f" % (i, got[i], fd))
        assert abs(got[i] - fd) <= 1e-6 * max(1.0, abs(fd))


def test_fp64_statement_agrees_with_the_long_double_one():
    """the two host statements of a small model: value and autograd gradients of the fp64 one against the long-double closed form,
    under the suite's floors (tests/_xref.FLOOR) -- what makes e64 a meaningful yardstick."""
    x, y = rng.make_regression(60, 2, 2, seed=43)
    ref, t64 = lo.make_pair(x, y, "Exp", 1.1, 0.9, 0.05, mean=[0.1, 0.2])
    loss, grads = t64.loss_grads_with_mean()
    assert xr.rel_err(loss, ref.loss()) <= xr.FLOOR["loss"]
    for g, want in zip(grads, ref.loss_grads()):
        assert xr.rel_err(g, want) <= xr.FLOOR["grad"]


def test_argument_validation_without_launch():
    """every gpn_loo_* entry point rejects bad arguments with -(argument index) / GPN_E_* before any HIP call (null pointers and a
    dummy host address throughout, as tests/test_abi.py does for its neighbours)."""
    import ctypes
    lib = _native.lib()
    null = None
    one = ctypes.c_double(0.0)
    p = ctypes.cast(ctypes.pointer(one), ctypes.c_void_p)
    # gpn_loo_terms(stream, n, dy, Kinv, ldk, at, ldat, work, work_bytes, qt, ldqt, var, rootd, value)
    assert lib.gpn_loo_terms(null, -1, 1, p, 4, p, 4, p, 8, null, 0, null, null, null) == -2
    assert lib.gpn_loo_terms(null, 4, 0, p, 4, p, 4, p, 8, null, 0, null, null, null) == -3
    assert lib.gpn_loo_terms(null, 4, 1, null, 4, p, 4, p, 8, null, 0, null, null, null) == -4
    assert lib.gpn_loo_terms(null, 4, 1, p, 3, p, 4, p, 8, null, 0, null, null, null) == -5
    assert lib.gpn_loo_terms(null, 4, 1, p, 4, null, 4, p, 8, null, 0, null, null, null) == -6
    assert lib.gpn_loo_terms(null, 4, 1, p, 4, p, 3, p, 8, null, 0, null, null, null) == -7
    assert lib.gpn_loo_terms(null, 4, 1, p, 4, p, 4, null, 8, null, 0, null, null, null) == -8
    assert lib.gpn_loo_terms(null, 257, 1, p, 257, p, 257, p, 8, null, 0, null, null, null) == -9       # two workgroups, one slot
    assert lib.gpn_loo_terms(null, 4, 1, p, 4, p, 4, p, 8, p, 3, null, null, null) == -11
    assert lib.gpn_loo_terms_work_bytes(1) == 8 and lib.gpn_loo_terms_work_bytes(257) == 16 and lib.gpn_loo_terms_work_bytes(0) == 0
    # gpn_loo_scale(stream, n, Kinv, ldk, rootd, S, lds)
    assert lib.gpn_loo_scale(null, -1, p, 4, p, p, 4) == -2
    assert lib.gpn_loo_scale(null, 4, null, 4, p, p, 4) == -3
    assert lib.gpn_loo_scale(null, 4, p, 3, p, p, 4) == -4
    assert lib.gpn_loo_scale(null, 4, p, 4, null, p, 4) == -5
    assert lib.gpn_loo_scale(null, 4, p, 4, p, null, 4) == -6
    assert lib.gpn_loo_scale(null, 4, p, 4, p, p, 3) == -7
    assert lib.gpn_loo_scale(null, 0, p, 0, p, p, 0) == 0                                               # nothing to do, nothing launched
    # gpn_loo_grad(stream, kind, X, n, d, variance, length_scales, nls, Q, ldq, at, ldat, wt, ldwt, dy, work, work_bytes, out)
    ok = lib.gpn_loo_grad_work_bytes(4, 1)
    assert ok == 3 * 8 and lib.gpn_loo_grad_work_bytes(129, 3) == 6 * 5 * 8 and lib.gpn_loo_grad_work_bytes(0, 1) == 0

    def grad(kind=0, X=p, n=4, d=2, var=p, ls=p, nls=1, Q=p, ldq=4, at=p, ldat=4, wt=p, ldwt=4, dy=1, work=p, wb=ok, out=p):
        return lib.gpn_loo_grad(null, kind, X, n, d, var, ls, nls, Q, ldq, at, ldat, wt, ldwt, dy, work, wb, out)

    assert grad(kind=6) == -2 and grad(kind=-1) == -2
    assert grad(X=null) == -3
    assert grad(n=-1) == -4
    assert grad(d=0) == -5
    assert grad(var=null) == -6
    assert grad(ls=null) == -7
    assert grad(nls=3) == -8
    assert grad(Q=null) == -9
    assert grad(ldq=3) == -10
    assert grad(at=null) == -11
    assert grad(ldat=3) == -12
    assert grad(wt=null) == -13
    assert grad(ldwt=3) == -14
    assert grad(dy=0) == -15
    assert grad(work=null) == -16
    assert grad(wb=ok - 8) == -17
    assert grad(out=null) == -18


def test_objective_keyword():
    x, y = rng.make_regression(20, 2, 1, seed=5)
    assert GPR(x, y, kernels.Rbf(2)).objective == "lml"
    assert GPR(x, y, kernels.Rbf(2), objective="loo").objective == "loo"
    for bad in ("bogus", "LOO", None):
        with pytest.raises(ValueError, match="objective"):
            GPR(x, y, kernels.Rbf(2), objective=bad)
    from gptorch_amd.models.dist_gpr import DistGPR
    with pytest.raises(NotImplementedError, match="leave-one-out"):
        DistGPR(x, y, kernels.Rbf(2), objective="loo")


def test_lockstep_grouping_leaves_loo_models_alone():
    """the grouping helpers of batched_loss_and_grad / multi_start_optimize never put a model with another objective into a group
    whose loss is formed as -(LML + log prior) (decided before anything touches a device: the filters come first)."""
    from gptorch_amd.models import _lockstep
    x, y = rng.make_regression(20, 2, 1, seed=5)
    ms = [GPR(x, y, kernels.Rbf(2)), GPR(x, y, kernels.Rbf(2), objective="loo"), GPR(x, y, kernels.Rbf(2))]
    assert _lockstep._lockstep_groups(ms, for_grad=True) == []           # (CPU-resident models form no group at all)
    masked = [m if m.objective == "lml" else None for m in ms]
    assert _lockstep._lockstep_groups(masked) == [] and _lockstep._expression_groups(masked) == []   # a masked entry is skipped, not an error
