"""Writes tests/golden/fitc_cases.json: the FITC golden cases (and, with --wide, tests/golden/fitc_wide_case.json: one case with
M > 1024, nothing else touched).  Inputs come from gptorch_amd.rng (regenerated from the seeds by
tests/_fitc_oracle.case_inputs), expected values from the host oracle tests/_fitc_oracle.py -- the dense N x N form in fp64
(loss, gradients by autograd) and in long double (loss, predictions), and the distance e64 between the two that the GPU
tests' tolerances are derived from (tests/_xref.tol).  Asserts on the way that K(Z) is well conditioned (no jitter ladder) and
that the closed-form backward of gptorch_amd/models/_fitc.py equals autograd through the dense form.

    python -m tests.golden.make_fitc_golden            # fitc_cases.json
    python -m tests.golden.make_fitc_golden --wide     # fitc_wide_case.json only (long double at N = 1400: about a minute)
"""
import json
import os
import sys

import numpy as np

from tests import _fitc_oracle as fo
from tests import _xref as xr

CASES = [
    dict(name="rbf_37x5", n=37, m=5, d=2, dy=1, kernel=dict(kind="Rbf", variance=1.1, length_scales=1.0), noise=0.1, seed_x=101, seed_xs=102),
    dict(name="matern52_ard_130x40x9", n=130, m=40, d=3, dy=9, kernel=dict(kind="Matern52", variance=1.2, length_scales=[0.9, 1.1, 1.3], ARD=True),
         noise=0.05, seed_x=111, seed_xs=112),
    dict(name="matern32_1000x200x3", n=1000, m=200, d=3, dy=3, kernel=dict(kind="Matern32", variance=1.3, length_scales=1.0), noise=0.1,
         seed_x=121, seed_xs=122),
    dict(name="composite_300x33", n=300, m=33, d=4, dy=2,
         kernel=dict(kind="Linear+Rbf+Constant", linear_variance=0.3, variance=1.1, length_scales=1.2, constant=0.5), noise=0.08,
         seed_x=131, seed_xs=132),
    dict(name="constant_mean_150x20", n=150, m=20, d=2, dy=2, kernel=dict(kind="Matern52", variance=0.9, length_scales=1.1), noise=0.06,
         mean=[0.3, -0.2], seed_x=141, seed_xs=142),
]
TRAJECTORY = dict(name="adam_130x40x9", n=130, m=40, d=3, dy=9, kernel=dict(kind="Matern52", variance=1.2, length_scales=[0.9, 1.1, 1.3], ARD=True),
                  noise=0.05, seed_x=111, seed_xs=112, steps=5, learning_rate=0.01)
# M > 1024 (a file of its own, written by --wide only): the <32> instantiation of the FITC forward row kernel and 18 column tiles
# of its backward; Z = the first 1100 rows of X, so lambda = noise on those rows
WIDE = dict(name="matern32_1400x1100x2", n=1400, m=1100, d=4, dy=2, kernel=dict(kind="Matern32", variance=1.3, length_scales=1.1), noise=0.08,
            seed_x=151, seed_xs=152)
# what every case carries (tests/test_fitc_host.py checks the file against it)
SCHEMA = ("name", "n", "m", "d", "dy", "kernel", "noise", "seed_x", "seed_xs", "cond_Kuu", "closed_form_err", "loss", "loss_ld", "e64",
          "grads", "mean_pred", "var_pred", "cov_pred")


def f64(a):
    return np.asarray(a, dtype=np.float64).tolist()


def make_case(case):
    inp = fo.case_inputs(case)
    o = fo.oracle_for(case, inp)
    out = dict(case)
    out["cond_Kuu"] = float(np.linalg.cond(o.K(o.raw["Z"]).detach().numpy()))
    assert out["cond_Kuu"] < 1e8, (case["name"], out["cond_Kuu"])
    out["closed_form_err"] = o.closed_form_check()
    assert out["closed_form_err"] < 1e-10, (case["name"], out["closed_form_err"])
    loss, grads = o.loss_and_grads()
    loss_ld = -o.lml_ld()
    mean, var = o.predict_f(inp["xs"])
    _, cov = o.predict_f(inp["xs"], diag=False)
    mean_ld, cov_ld = o.predict_ld(inp["xs"])
    out["loss"], out["loss_ld"] = loss, float(loss_ld)
    out["e64"] = dict(loss=xr.rel_err(loss, loss_ld), mean=xr.abs_err(mean, mean_ld), var=xr.abs_err(var, np.diag(cov_ld)),
                      cov=xr.abs_err(cov, cov_ld), grad=o.grad_e64())
    out["grads"] = {k: f64(v) for k, v in grads.items()}
    out["mean_pred"], out["var_pred"], out["cov_pred"] = f64(mean_ld), f64(np.diag(cov_ld)), f64(cov_ld)
    print("%-24s cond K(Z) %.1e  closed form %.1e  loss %.10f  e64 %s" % (case["name"], out["cond_Kuu"], out["closed_form_err"], loss,
                                                                          {k: "%.1e" % v for k, v in out["e64"].items()}))
    return out


def make_trajectory(t):
    inp = fo.case_inputs(t)
    out = dict(t)
    out["losses"] = fo.oracle_for(t, inp).optimize_adam(t["steps"], t["learning_rate"])
    print("trajectory", out["losses"])
    return out


def write(doc, name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


def main():
    write(dict(schema=list(SCHEMA), cases=[make_case(c) for c in CASES], trajectory=make_trajectory(TRAJECTORY)), "fitc_cases.json")


def main_wide():
    write(dict(schema=list(SCHEMA), cases=[make_case(WIDE)]), "fitc_wide_case.json")


if __name__ == "__main__":
    main_wide() if "--wide" in sys.argv[1:] else main()
