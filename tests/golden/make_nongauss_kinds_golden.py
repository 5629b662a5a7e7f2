#!/usr/bin/env python3
"""Writes tests/golden/nongauss_kinds_cases.npz: the EPGP model cases of tests/_nongauss_cases.py (Exp, Matern32, Periodic) from
the dense host EP oracle in long double -- loss, gradients, predict_f at 40 points -- with the fp64 oracle's distance e64 and its
sweep count beside them.  The sweep must converge in both arithmetics and B be positive definite at the fixed point.

    python tests/golden/make_nongauss_kinds_golden.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _nongauss_cases as nc  # noqa: E402


def main():
    out, meta = {}, {}
    for case in nc.EP_CASES:
        res = nc.ep_numbers(case)
        meta[case["name"]] = {"loss": res["loss"], "sweeps": res["sweeps"], "e64": res["e64"]}
        for key in ("grad_variance", "grad_length_scales", "mean", "var"):
            out["%s__%s" % (case["name"], key)] = res[key]
        print("%-28s loss %.12f sweeps %d e64 %s" % (case["name"], res["loss"], res["sweeps"], {k: "%.1e" % v for k, v in res["e64"].items()}))
    out["meta"] = np.array(json.dumps(meta))
    np.savez(os.path.join(ROOT, "tests", "golden", nc.GOLDEN_NAME), **out)


if __name__ == "__main__":
    main()
