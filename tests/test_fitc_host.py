"""FITC on the host (no GPU): the dense oracle against its long-double form on every golden case, the golden file against its
maker's schema and against a fresh oracle evaluation, what FITC is (not a VFE: never grouped into a lock-step VFE evaluation),
error paths, and argument validation of the gpn_fitc_* entry points."""
import numpy as np
import pytest
import torch

from gptorch_amd import _native, kernels, mean_functions
from gptorch_amd.models import FITC, VFE, _lockstep, sparse_gpr
from tests import _fitc_oracle as fo
from tests import _xref as xr
from tests._util import load_json
from tests.golden import make_fitc_golden as maker

CASES = load_json("fitc_cases.json")
WIDE = load_json("fitc_wide_case.json")
IDS = [c["name"] for c in CASES["cases"]]


@pytest.fixture(scope="module")
def evaluated():
    """name -> (inputs, oracle) of the golden cases, built once for the module."""
    out = {}
    for case in CASES["cases"]:
        inp = fo.case_inputs(case)
        out[case["name"]] = (inp, fo.oracle_for(case, inp))
    return out


@pytest.mark.parametrize("case", CASES["cases"], ids=IDS)
def test_dense_oracle_equals_long_double(case, evaluated):
    inp, o = evaluated[case["name"]]
    loss, grads = o.loss_and_grads()
    loss_ld = -o.lml_ld()
    mean, var = o.predict_f(inp["xs"])
    _, cov = o.predict_f(inp["xs"], diag=False)
    mean_ld, cov_ld = o.predict_ld(inp["xs"])
    errs = dict(loss=xr.rel_err(loss, loss_ld), mean=xr.rel_err(mean, mean_ld), var=xr.rel_err(var, np.diag(cov_ld)),
                cov=xr.rel_err(cov, cov_ld))
    print(case["name"], {k: "%.1e" % v for k, v in errs.items()})
    assert max(errs.values()) < 1e-10
    # ... and the file holds these values
    assert xr.rel_err(case["loss"], loss) < 1e-12 and xr.rel_err(case["loss_ld"], loss_ld) < 1e-12
    assert xr.abs_err(np.asarray(case["mean_pred"]), mean_ld) < 1e-12 and xr.abs_err(np.asarray(case["cov_pred"]), cov_ld) < 1e-12
    for k, g in grads.items():
        assert xr.rel_err(np.asarray(case["grads"][k]).reshape(g.shape), g) < 1e-11, k


def test_golden_file_matches_the_makers_schema():
    assert CASES["schema"] == list(maker.SCHEMA)
    assert [c["name"] for c in CASES["cases"]] == [c["name"] for c in maker.CASES]
    for case, spec in zip(CASES["cases"], maker.CASES):
        assert set(maker.SCHEMA) <= set(case)
        assert all(case[k] == v for k, v in spec.items())
        assert case["cond_Kuu"] < 1e8 and case["closed_form_err"] < 1e-10 and case["noise"] >= 0.05
        assert set(case["e64"]) == {"loss", "mean", "var", "cov", "grad"}
        assert set(case["grads"]) == set(fo.model_names(case))
        assert np.asarray(case["mean_pred"]).shape == (16, case["dy"]) and np.asarray(case["cov_pred"]).shape == (16, 16)
    shapes = {(c["n"], c["m"], c["d"], c["dy"], c["kernel"]["kind"]) for c in CASES["cases"]}
    assert {(37, 5, 2, 1, "Rbf"), (130, 40, 3, 9, "Matern52"), (1000, 200, 3, 3, "Matern32"), (300, 33, 4, 2, fo.COMPOSITE)} <= shapes
    assert any(c.get("mean") is not None for c in CASES["cases"])
    t = CASES["trajectory"]
    assert len(t["losses"]) == t["steps"] == 5 and all(a > b for a, b in zip(t["losses"], t["losses"][1:]))


def test_wide_golden_file_matches_the_makers_schema():
    """tests/golden/fitc_wide_case.json (make_fitc_golden.py --wide): one case with M > 1024, the schema of the others.  (Its
    long-double evaluation at N = 1400 is the maker's and is not repeated here.)"""
    assert WIDE["schema"] == list(maker.SCHEMA) and set(WIDE) == {"schema", "cases"} and len(WIDE["cases"]) == 1
    case, spec = WIDE["cases"][0], maker.WIDE
    assert set(maker.SCHEMA) <= set(case)
    assert all(case[k] == v for k, v in spec.items())
    assert case["m"] > 1024 and (case["n"], case["m"], case["d"], case["dy"], case["kernel"]["kind"]) == (1400, 1100, 4, 2, "Matern32")
    assert case["cond_Kuu"] < 1e8 and case["closed_form_err"] < 1e-10 and case["noise"] >= 0.05
    assert set(case["e64"]) == {"loss", "mean", "var", "cov", "grad"}
    assert set(case["grads"]) == set(fo.model_names(case))
    assert np.asarray(case["grads"]["Z"]).shape == (case["m"], case["d"])
    assert np.asarray(case["mean_pred"]).shape == (16, case["dy"]) and np.asarray(case["cov_pred"]).shape == (16, 16)
    assert np.isfinite(case["loss"]) and abs(xr.rel_err(case["loss"], case["loss_ld"]) - case["e64"]["loss"]) < 2.3e-16   # (loss_ld is stored rounded to fp64)
    inp = fo.case_inputs(case)                                                 # Z is the first M rows of X: lambda = noise there
    assert np.array_equal(inp["z"], inp["x"][:case["m"]])


def test_closed_form_backward_equals_autograd(evaluated):
    for name, (_, o) in evaluated.items():
        if o.X.shape[0] <= 300:
            assert o.closed_form_check() < 1e-10, name


def _small_model(cls=FITC, **kw):
    case = CASES["cases"][0]
    inp = fo.case_inputs(case)
    return cls(inp["x"], inp["y"], kernels.Rbf(case["d"]), inducing_points=inp["z"].copy(), **kw)


def test_fitc_is_not_a_vfe():
    m = _small_model()
    assert isinstance(m, sparse_gpr._InducingPointsGP) and not isinstance(m, VFE) and not issubclass(FITC, VFE)
    assert _lockstep._vfe_groups([m]) == []
    assert not m._can_capture("Adam")
    assert set(m.state_dict()) == {"Z", "kernel.variance", "kernel.length_scales", "likelihood.variance", "mean_function.val"}
    _small_model(mean_function=mean_functions.Constant(1))                     # mean functions are supported (VFE asserts)
    with pytest.raises(AssertionError):
        _small_model(VFE, mean_function=mean_functions.Constant(1))


def test_error_paths(monkeypatch):
    m = _small_model()
    with pytest.raises(ValueError, match="X and Y must have same # data."):
        m.log_likelihood(m.X[:10], m.Y)
    with pytest.raises(_native.NativeError):                                   # no CPU arithmetic behind the likelihood
        m.log_likelihood()
    monkeypatch.setattr(sparse_gpr, "SHARD_GROUP", True)
    with pytest.raises(NotImplementedError):
        m.log_likelihood()


def test_fitc_entry_points_validate_without_launch():
    lib = _native.lib()
    n = None
    one = 1 << 4                                                               # any non-null, 16-byte aligned address: nothing is launched
    assert lib.gpn_fitc_forward_work_bytes(0) == 0 and lib.gpn_fitc_forward_work_bytes(17) == 2 * 8 * 2

    def fwd(**kw):
        a = dict(At=one, lda=16, rows=4, m=10, err=one, dy=2, kdiag=one, kds=0, noise=0.1, errT=one, ldo=16, lam=one, work=one, out=one)
        a.update(kw)
        return lib.gpn_fitc_forward_rows(n, a["At"], a["lda"], a["rows"], a["m"], a["err"], a["dy"], a["kdiag"], a["kds"], a["noise"], a["errT"],
                                         a["ldo"], a["lam"], a["work"], a["out"])

    def bwd(**kw):
        a = dict(alpha=one, lda=16, T=one, ldt=32, rows=4, m=10, beta=one, ldb=2, dy=2, err=one, lam=one, r=one, g=one, aT=one, gaT=one, ldo=16)
        a.update(kw)
        return lib.gpn_fitc_backward_rows(n, a["alpha"], a["lda"], a["T"], a["ldt"], a["rows"], a["m"], a["beta"], a["ldb"], a["dy"], a["err"],
                                          a["lam"], a["r"], a["g"], a["aT"], a["gaT"], a["ldo"])
    assert fwd(At=None) == -2 and fwd(lda=8) == -3 and fwd(rows=0) == -4 and fwd(m=0) == -5 and fwd(err=None) == -6 and fwd(dy=0) == -7
    assert fwd(kdiag=None) == -8 and fwd(kds=-1) == -9 and fwd(noise=-1.0) == -10 and fwd(noise=float("nan")) == -10
    assert fwd(errT=None) == -11 and fwd(ldo=15) == -12 and fwd(rows=17, ldo=16) == -12 and fwd(lam=None) == -13
    assert fwd(work=None) == -14 and fwd(out=None) == -15 and fwd(lda=17) == -101 and fwd(At=one + 8) == -101
    assert bwd(alpha=None) == -2 and bwd(lda=8) == -3 and bwd(T=None) == -4 and bwd(ldt=16) == -5 and bwd(ldt=17) == -5
    assert bwd(rows=0) == -6 and bwd(m=0) == -7 and bwd(beta=None) == -8 and bwd(ldb=1) == -9 and bwd(dy=0) == -10
    assert bwd(err=None) == -11 and bwd(lam=None) == -12 and bwd(r=None) == -13 and bwd(g=None) == -14 and bwd(aT=None) == -15
    assert bwd(gaT=None) == -16 and bwd(ldo=15) == -17 and bwd(rows=17, ldo=16) == -17
    assert bwd(lda=17) == -101 and bwd(ldt=33) == -101 and bwd(ldo=17, rows=1) == -101 and bwd(T=one + 8) == -101
