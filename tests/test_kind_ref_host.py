"""CPU suite: the references of the kind-dispatch tests (tests/_kind_ref.py) and the widened fp64 branch of
tests/_laplace_oracle.kern, checked on the host.

  - kern in fp64 against tests/_xref.k_of_r2 in long double for every kind on the planted points, entries under the clamp having
    B exactly 0; the Rbf / Matern52 branches still give the bits they gave before Exp and Periodic were added;
  - the separation condition: for every output of every family the GPU tests check, the kinds' long-double references lie at
    least kr.SEPARATION tolerances of that output apart, pairwise -- a call served by another kind's instantiation fails."""
import itertools
import math

import numpy as np
import pytest

from gptorch_amd import rng
from tests import _kind_ref as kr
from tests import _laplace_oracle as lo
from tests import _refine_ref as rr
from tests import _xref as xr

LD = xr.LD


@pytest.mark.parametrize("d,ard", [(1, False), (2, True), (17, True)])
@pytest.mark.parametrize("kind", ["Rbf", "Matern52", "Matern32", "Exp", "Matern12", "Periodic"])
def test_fp64_kern_against_long_double_on_the_planted_points(kind, d, ard):
    n, var = 65, rr.VAR
    ls = np.atleast_1d(rr.length_scales(d, ard, 5 + d, 0.9)) * np.ones(d)
    x = rr.points(7 + d, n, d, ls[0])
    K64, B64 = lo.kern(kind, x, None, var, ls, np.float64)
    Kld, Bld = xr.k_of_r2(kind, xr.scaled_sqdist(x, None, ls), var)
    r2 = xr.scaled_sqdist(x, None, ls)
    dead = np.asarray(r2 < xr.CLAMP)
    assert dead.sum() > n                               # the planted repeated and 1e-21 pairs, beyond the diagonal
    if kind != "Rbf":
        assert np.all(B64[dead] == 0.0) and np.all(np.asarray(Bld)[dead] == 0)
    # fp64's r carries a relative error of (d + 2) u (d squares and sums, one square root), and every closed form a few
    # roundings of its own (64 u).  |dK/dr| <= 1.3 variance for every kind, so |dK| <= variance (64 + 1.3 (d + 2) r) u -- at the
    # planted r = 1000 Periodic's cos r feels the argument.  r |dB/dr| <= |B| (1 + 3 r) for the exponential kinds (Exp's
    # B = K / r: B (1 + r)) and <= 2 variance for Periodic's sin r / r, so |dB| <= (64 |B| + (d + 2) (|B| (1 + 3 r) + 2 variance)) u
    u = 2.0 ** -53
    r = np.sqrt(np.asarray(r2, dtype=np.float64))
    assert np.all(np.abs(K64.astype(LD) - Kld) <= var * (64 + 1.3 * (d + 2) * r) * u)
    live = ~dead
    absB = np.abs(np.asarray(Bld, dtype=np.float64))
    tolB = (64 * absB + (d + 2) * (absB * (1 + 3 * r) + 2 * var)) * u
    assert np.all(np.abs(B64.astype(LD) - Bld)[live] <= tolB[live])


def _old_kern64(kind, X, variance, ls):
    """the fp64 branch as it stood before this widening (Rbf, Matern52 only), restated: the same expressions in the same order."""
    r2 = np.zeros((X.shape[0], X.shape[0]))
    for c in range(X.shape[1]):
        t = (X[:, c:c + 1] - X[None, :, c]) / ls[c]
        r2 += t * t
    v = float(variance)
    if kind == "Rbf":
        K = v * np.exp(-0.5 * r2)
        return K, K.copy()
    dead = r2 < xr.CLAMP
    r = np.sqrt(np.maximum(r2, xr.CLAMP))
    e = np.exp(-math.sqrt(5.0) * r)
    K, B = v * (1.0 + math.sqrt(5.0) * r + 5.0 / 3.0 * r * r) * e, v * (5.0 / 3.0) * (1.0 + math.sqrt(5.0) * r) * e
    return K, np.where(dead, 0.0, B)


@pytest.mark.parametrize("kind", ["Rbf", "Matern52"])
def test_existing_oracle_kinds_keep_their_bits(kind):
    x = rng.normal(3, (40, 3))
    ls = np.array([0.8, 1.1, 1.4])
    got, want = lo.kern(kind, x, None, 1.3, ls, np.float64), _old_kern64(kind, x, 1.3, ls)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_every_entry_point_with_a_kernel_kind_is_in_the_table():
    """the table names exactly the entries of include/gpnative.h that take a kernel kind (the likelihood kinds of gpn_lik_* /
    gpn_ep_sites* are another enum)."""
    import os
    import re
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "gpnative.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = set(re.findall(r"\b(gpn_\w+)\s*\([^;]*?\bint kind\b", text))
    found = {f for f in found if not f.startswith(("gpn_lik_", "gpn_ep_"))}
    assert found == set(kr.SERVED), sorted(found ^ set(kr.SERVED))


def test_the_dispatch_inputs_are_factorable_for_every_covariance():
    """K + noise I of every model is positive definite in both arithmetics, the indefinite Periodic kernel at d = 2 included."""
    inp = kr.inputs()
    for b in range(inp.batch):
        var, ls, noise = inp.hyp(b)
        Kp = kr.kern("Periodic", inp.X, None, var, ls, np.float64)[0]
        assert np.linalg.eigvalsh(Kp).min() < -1.0                      # indefinite indeed
        for k in kr.COVARIANCES:
            kr.GP(kr.KIND_NAMES[k], b, np.float64)
            kr.GP(kr.KIND_NAMES[k], b, LD)


@pytest.mark.parametrize("family", list(kr.FAMILIES))
def test_kinds_are_separated_by_a_million_tolerances(family):
    kinds = kr.FAMILIES[family][1]
    worst = {}
    for b in range(kr.RAGGED_BATCH if family == "ragged" else kr.inputs().batch):
        refs = {k: kr.reference(family, k, b) for k in kinds}
        for k1, k2 in itertools.combinations(kinds, 2):
            for name, (v1, tol1, how) in refs[k1].items():
                v2, tol2, _ = refs[k2][name]
                gap = kr.metric(v1, v2, how) / max(tol1, tol2)
                worst[name] = min(worst.get(name, np.inf), gap)
                assert gap >= kr.SEPARATION, (family, name, kr.KIND_NAMES[k1], kr.KIND_NAMES[k2], b, gap)
    print("%s: smallest gap / tol per output %s" % (family, {k: "%.1e" % v for k, v in worst.items()}))


# ---- the inputs of tests/test_gpu_nongauss_kinds.py ---------------------------------------------------------------------------------------
from tests import _nongauss_cases as nc  # noqa: E402

SEPARABLE_TILE_CASES = [c for c in nc.TILE_CASES if c[1] > 1]


@pytest.mark.parametrize("kind,n,d,ard", SEPARABLE_TILE_CASES)
def test_tile_case_inputs_separate_the_kinds(kind, n, d, ard):
    """on the inputs of every tile case with n > 1, the five kinds' references of K, K v, diag and the gradient sweep differ
    pairwise by at least kr.SEPARATION tolerances: the case fails if the call ran any other kind's instantiation.  (n = 1 cannot
    separate: the one entry is k(x, x) = variance for every kind, and its length-scale gradient is 0 -- those four cases check
    the single-row path, not the kind.  The lock-step test compares bits with the single calls, which these cases judge.)"""
    t = nc.tile_inputs(kind, n, d, ard)
    refs = {k: nc.tile_refs(t, k) for k in nc.KINDS}
    for k1, k2 in itertools.combinations(nc.KINDS, 2):
        for name, (v1, tol1, how) in refs[k1].items():
            v2, tol2, _ = refs[k2][name]
            gap = kr.metric(v1, v2, how) / max(tol1, tol2)
            assert gap >= kr.SEPARATION, (name, k1, k2, gap)


def _other_kinds_losses(case, build, search):
    """the fp64 oracle's loss on the case's inputs under each kind (None where the oracle cannot factor or converge: an
    indefinite Periodic K at d >= 2 -- separated by failing)."""
    inp = nc.model_inputs(case)
    out = {}
    for k in nc.KINDS:
        try:
            out[k] = float(search(build(dict(case, kind=k), inp)).loss())
        except (np.linalg.LinAlgError, RuntimeError, FloatingPointError):
            out[k] = None
    return out


@pytest.mark.parametrize("case", nc.MODEL_CASES + nc.EP_CASES, ids=[c["name"] for c in nc.MODEL_CASES + nc.EP_CASES])
def test_model_case_inputs_separate_the_kinds(case):
    """the loss of every model case lies at least kr.SEPARATION tolerances from the loss the same inputs give under any other kind."""
    from tests import _ep_oracle as eo
    if case in nc.EP_CASES:
        losses = _other_kinds_losses(case, eo.build_oracle, lambda o: o.search(damping=nc.EP_DAMPING))
        e_loss = nc.ep_golden(case)["e64"]["loss"]
    else:
        losses = _other_kinds_losses(case, lo.build_oracle, lambda o: o.search())
        e_loss = nc.oracle_numbers(case)["e64"]["loss"]
    own = losses[case["kind"]]
    assert own is not None
    for k, v in losses.items():
        if k != case["kind"] and v is not None and np.isfinite(v):
            gap = abs(v - own) / max(1.0, abs(own)) / xr.tol(e_loss, "loss")
            assert gap >= kr.SEPARATION, (case["name"], k, gap)


@pytest.mark.parametrize("case", nc.EP_CASES, ids=[c["name"] for c in nc.EP_CASES])
def test_ep_fixture_matches_the_fp64_oracle(case):
    """the stored long-double numbers belong to the committed inputs: the fp64 oracle, run here, converges (B positive definite
    at the fixed point) and lies within the stored e64 of them."""
    from tests import _ep_oracle as eo
    gold = nc.ep_golden(case)
    o = eo.build_oracle(case, gold["inp"]).search(damping=nc.EP_DAMPING)
    assert not o.stalled and o.sweeps == gold["sweeps"] and np.all(np.diag(o.L) > 0)
    slack = 1.0 + 1e-6                                           # (the fixture holds the long-double numbers rounded to fp64)
    assert xr.rel_err(o.loss(), gold["loss"]) <= gold["e64"]["loss"] * slack + 2.0 ** -52
    g = o.loss_grads()
    assert max(xr.rel_err(g[0], gold["grad_variance"]), xr.rel_err(g[1], gold["grad_length_scales"])) <= gold["e64"]["grad"] * slack + 2.0 ** -52
    mean, var = o.predict_f(gold["inp"]["xs"])
    assert xr.abs_err(mean, gold["mean"]) <= gold["e64"]["mean"] * slack + 2.0 ** -52
    assert xr.abs_err(var, gold["var"]) <= gold["e64"]["var"] * slack + 2.0 ** -52
