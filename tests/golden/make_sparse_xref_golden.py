"""Writes tests/golden/sparse_xref_cases.json and tests/golden/fitc_xref_cases.json: the long-double references of the cases of
tests/_sparse_ref.VFE_CASES / FITC_CASES that are too large to evaluate inside a test (golden=True: N = 4700, M = 1153, whose
A A^T alone is 6e9 long-double multiply-adds).  Inputs are regenerated from the case's seed by tests/_sparse_ref.case_inputs; a
file holds the loss, every gradient, the predictions at the case's 16 points and e64, the distance of the plain fp64 evaluation
(tests/_sparse_ref.Direct64VFE / Direct64FITC) from the long-double one that the GPU test's tolerances are derived from
(tests/_xref.tol).  Values are the long-double results rounded to fp64 (1e-16 relative, six orders below the tightest tolerance).

    python -m tests.golden.make_sparse_xref_golden          # both files, a few minutes each
    python -m tests.golden.make_sparse_xref_golden fitc     # fitc_xref_cases.json only (vfe: sparse_xref_cases.json only)
"""
import json
import os
import sys
import time

import numpy as np

from tests import _sparse_ref as sr

SCHEMA = ("name", "n", "m", "d", "dy", "kernel", "noise", "seed", "loss", "grads", "mean_pred", "var_pred", "cov_pred", "e64")
FAMILIES = {"vfe": (sr.VFE_CASES, sr.vfe_reference, "sparse_xref_cases.json"), "fitc": (sr.FITC_CASES, sr.fitc_reference, "fitc_xref_cases.json")}


def f64(a):
    return np.asarray(a, dtype=np.float64).tolist()


def make_case(case, reference=sr.vfe_reference):
    t = time.time()
    inp = sr.case_inputs(case)
    r = reference(case, inp)
    out = {k: case[k] for k in SCHEMA[:8]}
    out["loss"] = float(r["loss"])
    out["grads"] = {k: f64(g) for k, g in r["grads"].items()}
    out["mean_pred"], out["var_pred"], out["cov_pred"] = f64(r["mean"]), f64(r["var"]), f64(r["cov"])
    out["e64"] = r["e64"]
    print("%-20s %.0f s  loss %.10f  e64 %s" % (case["name"], time.time() - t, out["loss"],
                                               {k: "%.1e" % v for k, v in r["e64"].items() if k != "grads"}))
    return out


def main(families):
    for fam in families:
        cases, reference, name = FAMILIES[fam]
        doc = dict(schema=list(SCHEMA), cases=[make_case(c, reference) for c in cases if c.get("golden")])
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name)
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:] or list(FAMILIES))
