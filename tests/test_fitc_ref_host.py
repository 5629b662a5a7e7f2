"""tests/_sparse_ref.FITCRef is checked here, on the host, before tests/test_gpu_fitc_xref.py lets it judge the native path (the
conventions, the step rule of the central differences, the cap and the distance measure are those of tests/test_sparse_ref_host.py):

  - the likelihood and the predictions against the DENSE N x N long-double statement of tests/_fitc_oracle.py (lml_ld, predict_ld),
    which shares neither the whitening nor lambda with FITCRef's M-sized form;
  - every long-double gradient against central differences of the long-double likelihood and against fp64 autograd through the dense
    form (FITCOracle.loss_and_grads);
  - independence of the order of the rows of x;
  - FITCRef against the committed goldens of tests/golden/fitc_cases.json, at their stored tolerances;
  - the cap on every case's tolerances, and that the floors ARE the tolerances except where K(Z) is ill conditioned on purpose;
  - resolving power: a reference evaluated WITH a planted mistake lies at least 100 tolerances from the true one.

Each test prints its figures (pytest -s)."""
import functools

import numpy as np
import pytest

from tests import _fitc_oracle as fo
from tests import _sparse_ref as sr
from tests import _xref as xr
from tests import test_sparse_ref_host as base
from tests._util import load_json

LD = xr.LD
CAP = base.CAP
FITC = {c["name"]: c for c in sr.FITC_CASES}
GOLDEN = load_json("fitc_cases.json")
# the cases whose K(Z) is ill conditioned by construction (cond ~ 1e8, and two identical inducing points): 16 e64 stands above the floors
ABOVE_FLOORS = ("inverse_knob_ignored", "ladder")


@functools.lru_cache(maxsize=None)
def inputs(name):
    return sr.case_inputs(FITC[name])


@functools.lru_cache(maxsize=None)
def reference(name):
    """what the GPU tests hold the native path to: dict(loss, grads, mean, var, cov, e64) -- the golden case from its fixture."""
    case, inp = FITC[name], inputs(name)
    if case.get("golden"):
        g = {c["name"]: c for c in load_json("fitc_xref_cases.json")["cases"]}[name]
        assert all(g[k] == case[k] for k in ("n", "m", "d", "dy", "kernel", "noise", "seed"))
        return dict(loss=g["loss"], grads=g["grads"], mean=g["mean_pred"], var=g["var_pred"], cov=g["cov_pred"], e64=g["e64"])
    return sr.fitc_reference(case, inp, jitter=base.host_jitter(case, inp))


# ---- the dense N x N statement -----------------------------------------------------------------------------------------
# Both sides are long double (eps = 2^-63 = 1.1e-19); the dense side factors an N x N matrix whose condition number is at most
# (N max Kdiag + s) / s < 1e5 for these cases, and sums N M products: 1e-14 leaves four decimal digits over eps cond sqrt(N M) and
# is 1e-4 of the tightest floor the reference is used with.
DENSE_CASES = ["dy_across_16", "one_chunk", "composite"]


@pytest.mark.parametrize("name", DENSE_CASES)
def test_reference_against_the_dense_long_double_statement(name):
    case, inp = FITC[name], inputs(name)
    assert sorted(c["n"] for c in sr.FITC_CASES if not c.get("ladder"))[:3] == sorted(FITC[k]["n"] for k in DENSE_CASES)
    ref = sr.fitc_refs(case, inp)[0]
    o = fo.FITCOracle(inp["x"], inp["y"], inp["z"], case["kernel"], case["noise"], mean=case.get("mean"))
    mu, cov = o.predict_ld(inp["xs"])
    m1, var = ref.predict_f(inp["xs"], True)
    m2, c2 = ref.predict_f(inp["xs"], False)
    errs = (xr.rel_err(ref.loss(), -o.lml_ld()), xr.abs_err(m1, mu), xr.abs_err(m2, mu), xr.abs_err(var, np.repeat(np.diag(cov)[:, None], case["dy"], 1)),
            xr.abs_err(c2, cov))
    print("fitc/%s against the dense form: loss %.2e  mean %.2e / %.2e  var %.2e  cov %.2e" % ((name,) + errs))
    assert max(errs) <= 1e-14, errs


# ---- gradients: central differences in long double (the rule of tests/test_sparse_ref_host.py) ------------------------------------
def _build(case, inp, th):
    return sr.FITCRef(inp["x"], inp["y"], th["Z"], base._kernel_of(case, th), np.exp(th["noise"])[0], mean=th["mean"])


FD_CASES = ["one_chunk", "m_odd_across_a_leaf", "dy_across_16", "composite"]


@pytest.mark.parametrize("name", FD_CASES)
def test_gradients_against_central_differences(name):
    """every block of the long-double gradient (the Constant mean included) against Richardson-extrapolated central differences of
    the long-double likelihood along a random direction: |g.u - D*(h)| <= 100 EPS_EFF^(4/5) max(1, |F|) + |D*(h) - D*(2h)|."""
    case, inp = FITC[name], inputs(name)
    mean = case.get("mean") or list(0.3 - 0.25 * np.arange(case["dy"]))
    th = base._theta(case, inp, mean, False)
    ref = _build(case, inp, th)
    F, g = ref.loss(), ref.loss_grads()
    assert set(g) == set(th)
    eps = base._eps_eff(ref.n, ref.m)
    h = LD(eps ** 0.2)
    bound = 100.0 * eps ** 0.8 * max(1.0, abs(float(F)))
    print("fitc/%s: |F| %.3e  h %.2e  bound %.2e" % (name, abs(float(F)), float(h), bound))
    for k, u in base._directions(th, ref.X, 7).items():
        def along(t):
            return _build(case, inp, dict(th, **{k: th[k] + t * u})).loss()
        D = [(along(t * h) - along(-t * h)) / (2 * t * h) for t in (1, 2, 4)]
        Ds, Ds2 = (4 * D[0] - D[1]) / 3, (4 * D[1] - D[2]) / 3
        gu = np.sum(xr.ld(g[k]).reshape(u.shape) * u)
        err, trunc = abs(float(gu - Ds)), abs(float(Ds - Ds2))
        print("   d/d%-16s g.u %+.12e  central %+.12e  |diff| %.2e (%.1e of |g.u|; bound %.1e + %.1e)"
              % (k, float(gu), float(Ds), err, err / max(abs(float(gu)), 1e-300), bound, trunc))
        assert err <= bound + trunc, "%s: closed form %.15e, central differences %.15e, |diff| %.2e > %.2e" % (k, float(gu), float(Ds), err, bound + trunc)


# ---- gradients: fp64 autograd through the dense form -----------------------------------------------------------------------
# (the dense form builds and differentiates an N x N factorisation: the cases up to N = 1300; the two N = 8.2k / 8.6k cases and the
# fixture case are held by the M-sized autograd behind e64, below.  The ladder case has no dense statement: K(Z) is singular.)
DENSE_GRAD_CASES = [c["name"] for c in sr.FITC_CASES if c["n"] <= 1300 and not c.get("ladder")]


@pytest.mark.parametrize("name", DENSE_GRAD_CASES)
def test_gradients_against_fp64_autograd_of_the_dense_form(name):
    """every block within CAP / 16 = 6.25e-9 relative of autograd through the N x N form, the distance the cap of
    tests/test_sparse_ref_host.py leaves between the long-double gradient and an fp64 derivation."""
    case, inp, r = FITC[name], inputs(name), reference(name)
    o = fo.FITCOracle(inp["x"], inp["y"], inp["z"], case["kernel"], case["noise"], mean=case.get("mean"))
    loss, g = o.loss_and_grads()
    assert set(g) == set(fo.model_names(case))
    print("fitc/%s against dense autograd: loss %.2e" % (name, xr.rel_err(loss, r["loss"])))
    assert xr.rel_err(loss, r["loss"]) <= CAP["loss"] / xr.SAFETY
    for k, v in g.items():
        err = xr.rel_err(v.reshape(np.shape(r["grads"][k])), r["grads"][k])
        print("   d/d%-19s rel err %.2e (bound %.2e)" % (k, err, CAP["grad"] / xr.SAFETY))
        assert err <= CAP["grad"] / xr.SAFETY, k


@pytest.mark.parametrize("name", [c["name"] for c in sr.FITC_CASES])
def test_e64_and_the_cap(name):
    """e64 is the distance of the M-sized fp64 evaluation (gradients: autograd through it) from the long-double one.  On every case
    but the ladder one the derived tolerance xr.tol(e64, what) is no wider than the fixed tolerance the suite used so far (1e-8 / 1e-7 /
    1e-8); on every case whose K(Z) is not ill conditioned on purpose 16 e64 is below the floor, so the floors are the tolerances."""
    case, r = FITC[name], reference(name)
    e = r["e64"]
    print("fitc/%s" % name)
    for what in ("loss", "mean", "var"):
        print("   %-22s e64 %.2e  tol %.2e  cap %.0e" % (what, e[what], xr.tol(e[what], what), CAP[what]))
    for k, v in e["grads"].items():
        print("   d/d%-19s e64 %.2e  tol %.2e  cap %.0e" % (k, v, xr.tol(v, "grad"), CAP["grad"]))
    want = {"variance", "length_scales", "noise", "mean", "Z"} | ({"linear_variance", "constant"} if case["kernel"]["kind"] == sr.COMPOSITE else set())
    assert want <= set(e["grads"]) and want <= set(r["grads"])
    if case.get("ladder"):
        return
    for what in ("loss", "mean", "var"):
        assert xr.tol(e[what], what) <= CAP[what], (what, e[what])
        assert name in ABOVE_FLOORS or xr.tol(e[what], what) == xr.FLOOR[what], (what, e[what])
    for k, v in e["grads"].items():
        assert xr.tol(v, "grad") <= CAP["grad"], (k, v)
        assert name in ABOVE_FLOORS or xr.tol(v, "grad") == xr.FLOOR["grad"], (k, v)


# ---- the order of the rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m_odd_across_a_leaf", "ragged_multi_chunk", "composite"])
def test_reference_does_not_depend_on_the_row_order(name):
    """the rows of x permuted: only the order of the N-sized sums changes, so the distance between the two evaluations is the
    reference's own rounding -- 1e-13 relative for the likelihood and every gradient block, 1e-4 of the tightest floor."""
    case, inp = FITC[name], inputs(name)
    p = np.random.RandomState(5).permutation(case["n"])
    refs = [sr.FITCRef(inp["x"][rows], inp["y"][rows], inp["z"], case["kernel"], case["noise"], mean=case.get("mean")) for rows in (np.arange(case["n"]), p)]
    d = {"loss": xr.rel_err(refs[1].loss(), refs[0].loss())}
    g0, g1 = refs[0].loss_grads(), refs[1].loss_grads()
    d.update({k: xr.rel_err(g1[k], g0[k]) for k in g0})
    print("fitc/%s rows permuted: " % name + "  ".join("%s %.1e" % kv for kv in d.items()))
    assert max(d.values()) <= 1e-13, d


# ---- the committed goldens ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_reference_against_the_committed_goldens(g):
    """the new reference and the dense oracle behind tests/golden/fitc_cases.json state the same model: the long-double loss and
    predictions of the golden cases (Z a subset of the rows of x) at the tolerances tests/test_gpu_fitc.py derives from their stored
    e64, the stored fp64 autograd gradients at theirs."""
    inp = fo.case_inputs(g)
    ref = sr.FITCRef(inp["x"], inp["y"], inp["z"], g["kernel"], g["noise"], mean=g.get("mean"))
    e = g["e64"]
    mu, var = ref.predict_f(inp["xs"], True)
    _, cov = ref.predict_f(inp["xs"], False)
    errs = (xr.rel_err(ref.loss(), g["loss_ld"]), xr.abs_err(mu, g["mean_pred"]), xr.abs_err(var[:, 0], g["var_pred"]), xr.abs_err(cov, g["cov_pred"]))
    tols = (xr.tol(e["loss"], "loss"), xr.tol(e["mean"], "mean"), xr.tol(e["var"], "var"), xr.tol(e["cov"], "var"))
    print("fitc golden %s: loss %.2e (tol %.1e)  mean %.2e (%.1e)  var %.2e (%.1e)  cov %.2e (%.1e)" % ((g["name"],) + tuple(v for p in zip(errs, tols) for v in p)))
    assert all(a <= t for a, t in zip(errs, tols)), (errs, tols)
    grads = ref.loss_grads()
    for k in fo.model_names(g):
        err = xr.rel_err(np.asarray(g["grads"][k]).reshape(np.shape(grads[k])), grads[k])
        print("   d/d%-19s rel err %.2e (tol %.1e)" % (k, err, xr.tol(e["grad"], "grad")))
        assert err <= xr.tol(e["grad"], "grad"), k


# ---- resolving power ---------------------------------------------------------------------------------------------------
# (case, mistake, where, the quantities of the GPU check the mistake has to move by at least 100 of their tolerances); every case is
# one tests/test_gpu_fitc_xref.py runs under the route the mistake mimics: six chunks with a ragged tail on one and two lanes, and
# the composite kernel's per-chunk Kdiag slices
PLANTS = [
    ("ragged_multi_chunk", "drop_last_row", 0, ("loss", "grad", "mean")),                      # mean: predict_f's mean AND variance
    ("ragged_multi_chunk", "sums_first_chunk", 256, ("loss", "grad", "grad:noise")),
    ("ragged_multi_chunk", "aga_triangle", 0, ("grad", "grad:length_scales", "grad:Z")),
    ("ragged_multi_chunk", "drop_kdiag_grad", 0, ("grad", "grad:variance")),
    ("composite", "drop_kdiag_grad", 0, ("grad", "grad:variance", "grad:linear_variance", "grad:constant")),
    ("ragged_multi_chunk", "g_without_h", 0, ("grad", "grad:noise", "grad:variance")),
]


@pytest.mark.parametrize("name,plant,at,quantities", PLANTS, ids=["%s-%s" % p[:2] for p in PLANTS])
def test_resolving_power(name, plant, at, quantities):
    """a reference evaluated with the mistake planted lies at least 100 tolerances from the true one, in every quantity listed (a
    mistake in the backward alone leaves the loss and the predictions where they are)."""
    case, inp, true = FITC[name], inputs(name), reference(name)
    assert set(sr.FITC_PLANTS) == set(p[1] for p in PLANTS)
    planted = sr.fitc_refs(case, inp, plant=plant, plant_at=at)[0]
    d = base._distance(planted, true, true["e64"], inp["xs"], quantities)
    print("fitc/%s with %s: " % (name, plant) + "  ".join("%s %.1e tol" % kv for kv in d.items()))
    assert all(v >= 100.0 for v in d.values()), d
