"""Goldens of the leave-one-out objective of GPR (gptorch_amd/csrc/loo.hip, GPR(objective="loo")) -> tests/golden/loo_cases.npz.
CPU only:

    python tests/golden/make_loo_golden.py

Per case (tests/_loo_oracle.py; inputs from gptorch_amd.rng): the long-double loss -L_LOO, its gradients w.r.t. (log variance,
log length_scales, log noise, mean), the leave-one-out means and variances of every point, and for each quantity e64, the
distance of the plain-fp64 statement (LooTorch: dense LAPACK inverse, autograd) from the long-double one -- never a distance
to the code under test.  e64["dense_grad"] is that distance for the matrix G, entrywise (G itself is not stored: the tests
re-evaluate it from the oracle).  For the first case also the means and variances of 300 REFITS, each on the 299 other points.

A case whose 16 e64 exceeds 1e-6 for any quantity pins nothing and is refused.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gptorch_amd import rng  # noqa: E402
from tests import _loo_oracle as lo  # noqa: E402
from tests import _xref as xr  # noqa: E402

CASES = [
    dict(name="rbf_300x2", kind="Rbf", n=300, d=2, dy=1, ARD=False, variance=1.3, length_scales=[0.8], noise=0.05, mean=None, seed=211,
         refits=True),
    dict(name="matern52_ard_257x3", kind="Matern52", n=257, d=3, dy=2, ARD=True, variance=1.6, length_scales=[1.1, 0.7, 1.5], noise=0.02,
         mean=[0.3, -0.2], seed=223, refits=False),
    # dy = 5: the gradient sweep stages a^T and w^T four right-hand sides at a time, so this case crosses into a second pass
    dict(name="exp_513x2_dy5", kind="Exp", n=513, d=2, dy=5, ARD=False, variance=0.9, length_scales=[1.2], noise=0.05, mean=None, seed=227,
         refits=False),
]
REFUSE_ABOVE = 1e-6


def case_inputs(case):
    return rng.make_regression(case["n"], case["d"], case["dy"], seed=case["seed"])


def build(case, inputs=None):
    x, y = case_inputs(case) if inputs is None else inputs
    ls = case["length_scales"] if case["ARD"] else case["length_scales"][0]
    return lo.make_pair(x, y, case["kind"], case["variance"], ls, case["noise"], ARD=case["ARD"], mean=case["mean"])


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
    m64, v64 = t64.loo_predict()
    mld, vld = ref.loo_predict()
    e64["mean"], e64["var"] = xr.abs_err(m64, mld), xr.abs_err(v64, vld)
    res["mean"], res["var"] = np.asarray(mld, dtype=np.float64), np.asarray(vld, dtype=np.float64)
    (G64, w64), (Gld, wld) = t64.G(), ref.G()
    e64["dense_grad"] = max(xr.abs_err(G64, Gld), xr.abs_err(w64, wld))
    res["e64"] = e64
    if case["refits"]:
        fits = [ref.refit(i) for i in range(case["n"])]
        res["refit_mean"] = np.asarray([f[0] for f in fits], dtype=np.float64)
        res["refit_var"] = np.asarray([f[1] for f in fits], dtype=np.float64)
        worst = max(xr.rel_err(np.asarray([f[0] for f in fits]), mld), xr.rel_err(np.asarray([f[1] for f in fits]), vld[:, 0]))
        print("%-22s closed form vs %d refits (long double): %.2e" % (case["name"], case["n"], worst))
    print("%-22s loss %.10f e64 %s" % (case["name"], res["loss"], {k: "%.1e" % v for k, v in e64.items()}))
    bad = {k: v for k, v in e64.items() if xr.SAFETY * v > REFUSE_ABOVE}
    if bad:
        raise SystemExit("case %s pins nothing: 16 e64 > %g for %s" % (case["name"], REFUSE_ABOVE, bad))
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
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "loo_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
