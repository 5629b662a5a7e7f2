"""Goldens of the k-fold objective of GPR (gptorch_amd/csrc/kfold.hip, GPR(objective="kfold")) -> tests/golden/kfold_cases.npz.
CPU only:

    python tests/golden/make_kfold_golden.py

Generated from the host oracle (tests/_kfold_oracle.py; inputs from gptorch_amd.rng): the reference project has no
cross-validation.  Per case: the folds, the long-double loss -L_kfold, its gradients w.r.t. (log variance, log length_scales,
log noise, mean), the held-out means and variances of every point in closed form, for the first and the last fold the means and
variances of a REFIT on the other folds, and for each quantity e64, the distance of the plain-fp64 statement (KFoldTorch: dense
LAPACK inverse, autograd) from the long-double one -- never a distance to the code under test.

Asserted here for every case: (a) closed form = refit, fold by fold and summed: the value to 1e-15 relative, means and variances to
1e-14, both sides in long double; (b) 16 e64 <= 1e-7 for loss, mean and var and <= 1e-6 for the gradients, so that the tolerances
the tests derive from e64 pin something.  A case that violates (b) is changed, not the cap: noise >= 1e-2 variance, length scales
of order sqrt(d).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gptorch_amd import rng  # noqa: E402
from tests import _kfold_oracle as ko  # noqa: E402
from tests import _xref as xr  # noqa: E402

# folds: an int k, or {"sizes": [...], "shuffle": seed or None} (None: contiguous blocks of those sizes in data order)
CASES = [
    dict(name="rbf_7x1_k2", kind="Rbf", n=7, d=1, dy=1, ARD=False, variance=1.3, length_scales=[1.0], noise=0.05, mean=None, seed=311,
         folds=2),
    dict(name="matern52_ard_64x8_32_32", kind="Matern52", n=64, d=8, dy=2, ARD=True, variance=1.6,
         length_scales=[2.5, 3.0, 2.8, 3.3, 2.6, 3.1, 2.9, 2.7], noise=0.05, mean=[0.3, -0.2], seed=313, folds=dict(sizes=[32, 32], shuffle=None)),
    # a singleton fold next to a 63-point one; dy = 5 crosses the 4-at-a-time staging of a^T / w^T, d = 17 the 16-coordinate staging
    dict(name="exp_64x17_63_1_dy5", kind="Exp", n=64, d=17, dy=5, ARD=False, variance=0.9, length_scales=[4.0], noise=0.05, mean=None, seed=317,
         folds=dict(sizes=[63, 1], shuffle=None)),
    dict(name="matern32_ard_65x17_k4", kind="Matern32", n=65, d=17, dy=1, ARD=True, variance=1.1,
         length_scales=[4.0 + 0.1 * i for i in range(17)], noise=0.03, mean=None, seed=331, folds=4),
    dict(name="rbf_ard_203x8_shuffled_dy5", kind="Rbf", n=203, d=8, dy=5, ARD=True, variance=1.3,
         length_scales=[2.6, 3.1, 2.7, 3.4, 2.9, 3.0, 2.8, 3.2], noise=0.05, mean=[0.1, -0.1, 0.2, 0.0, 0.3], seed=337,
         folds=dict(sizes=[64, 65, 48, 26], shuffle=339)),
    dict(name="exp_203x1_k6", kind="Exp", n=203, d=1, dy=2, ARD=False, variance=0.9, length_scales=[1.2], noise=0.05, mean=[0.2, -0.3], seed=347,
         folds=6),
    # 129 / 128 / 43: crosses the 128-row leaf of the fold factorisations and the 16 / 64 tile edges
    dict(name="matern52_300x17_shuffled", kind="Matern52", n=300, d=17, dy=1, ARD=False, variance=1.6, length_scales=[4.2], noise=0.04, mean=None,
         seed=349, folds=dict(sizes=[129, 128, 43], shuffle=353)),
]
CAP = {"loss": 1e-7, "mean": 1e-7, "var": 1e-7, "grad": 1e-6}
REFIT_VALUE, REFIT_PRED = 1e-15, 1e-14


def case_inputs(case):
    return rng.make_regression(case["n"], case["d"], case["dy"], seed=case["seed"])


def case_folds(case):
    """an int k as it stands, else the list of index arrays"""
    f = case["folds"]
    if isinstance(f, int):
        return f
    order = np.arange(case["n"]) if f["shuffle"] is None else np.argsort(rng.uniform(f["shuffle"], case["n"]), kind="stable")
    assert sum(f["sizes"]) == case["n"]
    return [np.asarray(p, dtype=np.int64) for p in np.split(order, np.cumsum(f["sizes"])[:-1])]


def build(case, inputs=None):
    x, y = case_inputs(case) if inputs is None else inputs
    ls = case["length_scales"] if case["ARD"] else case["length_scales"][0]
    return ko.make_pair(x, y, case["kind"], case["variance"], ls, case["noise"], ARD=case["ARD"], mean=case["mean"], folds=case_folds(case))


def model_case(case):
    ref, t64 = build(case)
    res, e64 = {}, {}
    loss64, g64 = t64.loss_grads_with_mean()
    res["loss"] = float(ref.loss())
    e64["loss"] = xr.rel_err(loss64, ref.loss())
    gld = ref.loss_grads()
    e64["grad"] = max(xr.rel_err(a, b) for a, b in zip(g64, gld))
    for nm, g in zip(("variance", "length_scales", "noise", "mean"), gld):
        res["grad_" + nm] = np.asarray(g, dtype=np.float64)
    m64, v64 = t64.kfold_predict()
    mld, vld = ref.kfold_predict()
    e64["mean"], e64["var"] = xr.abs_err(m64, mld), xr.abs_err(v64, vld)
    res["mean"], res["var"] = np.asarray(mld, dtype=np.float64), np.asarray(vld, dtype=np.float64)
    res["e64"] = e64
    res["folds_idx"] = np.concatenate(ref.parts)
    res["folds_off"] = np.concatenate([[0], np.cumsum([p.size for p in ref.parts])])
    # (a) the closed form against real refits, every fold, both sides in long double
    total, worst = xr.LD(0), 0.0
    k = len(ref.parts)
    for f, I in enumerate(ref.parts):
        logp, mean, var = ref.refit(f)
        total += logp
        assert abs(logp - ref.fold_log_density(f)) <= REFIT_VALUE * max(1, abs(logp)), (case["name"], f)
        worst = max(worst, xr.rel_err(mean, mld[I]), xr.rel_err(var, vld[I, 0]))
        if f in (0, k - 1):
            tag = "first" if f == 0 else "last"
            res["refit_%s_mean" % tag], res["refit_%s_var" % tag] = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    dv = float(abs(total - ref.kfold()) / max(1, abs(ref.kfold())))
    print("%-30s closed form vs %d refits (long double): value %.2e, mean / var %.2e" % (case["name"], k, dv, worst))
    assert dv <= REFIT_VALUE and worst <= REFIT_PRED, case["name"]
    print("%-30s loss %.10f e64 %s" % (case["name"], res["loss"], {k: "%.1e" % v for k, v in e64.items()}))
    # (b) the derived tolerances pin something
    bad = {k: v for k, v in e64.items() if xr.SAFETY * v > CAP[k]}
    if bad:
        raise SystemExit("case %s: 16 e64 above the cap for %s -- change the case, not the cap" % (case["name"], bad))
    return res


def main():
    out, meta = {}, {"cases": []}
    for case in CASES:
        res = model_case(case)
        entry = dict(case)
        for k, v in res.items():
            if isinstance(v, np.ndarray):
                out["%s__%s" % (case["name"], k)] = v
            else:
                entry[k] = v
        meta["cases"].append(entry)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kfold_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
