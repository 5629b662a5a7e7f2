"""Goldens of LaplaceGP (gptorch_amd/models/laplace.py, csrc/laplace.hip) -> tests/golden/laplace_cases.npz.  CPU only:

    python tests/golden/make_laplace_golden.py

(a) Pointwise: lp = log p(y | f), d1 = dlp/df, W = -d2lp/df2, d3 = d3lp/df3 from their DEFINITIONS in 40-digit arithmetic
    (mpmath, as make_lik_golden.py), Bernoulli at f in [-12, 12] for both labels and both links, Poisson at f in [-20, 10] with
    counts up to 10^4; beside each number the error e64 of the oracle's plain-fp64 closed form (tests/_laplace_oracle.derivs64).
(b) Model cases (tests/_laplace_oracle.py: dense K; inputs from gptorch_amd.rng): the long-double loss (iterated until
    max |delta f| stops shrinking), its gradients w.r.t. every raw parameter and the mean, predict_f mean / variance / covariance
    at 40 points, and for each the distance e64 of the plain-fp64 statement; the fp64 statement's Newton steps and halvings
    under the package's stopping rule.
(c) Ten steps of torch's CPU Adam on the fp64 statement of one case.

The generator asserts that every case converges in <= 20 steps and that a Poisson case halves a step at least once.
"""
import json
import os
import sys

import mpmath as mp
import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _laplace_oracle as lo  # noqa: E402
from tests import _xref as xr  # noqa: E402

CASES = [
    dict(name="probit_rbf_300x2", lik="probit", kind="Rbf", n=300, d=2, ARD=False, variance=1.7, length_scales=[0.9], mean=None, seed=101),
    dict(name="probit_matern52_ard_513x3", lik="probit", kind="Matern52", n=513, d=3, ARD=True, variance=2.2, length_scales=[1.1, 0.8, 1.6],
         mean=0.3, seed=103),
    dict(name="logit_rbf_ard_513x2", lik="logit", kind="Rbf", n=513, d=2, ARD=True, variance=3.0, length_scales=[0.7, 1.3], mean=None, seed=107),
    dict(name="logit_matern52_300x3", lik="logit", kind="Matern52", n=300, d=3, ARD=False, variance=1.4, length_scales=[1.2], mean=-0.2, seed=109),
    # a rate offset of e^1 and counts up to about 40: plain Newton from a = 0 overshoots, the step is halved
    dict(name="poisson_rbf_513x2", lik="poisson", kind="Rbf", n=513, d=2, ARD=False, variance=1.2, length_scales=[1.0], mean=None, seed=113,
         offset=1.0, gain=1.2),
    dict(name="poisson_matern52_ard_300x3", lik="poisson", kind="Matern52", n=300, d=3, ARD=True, variance=0.8, length_scales=[1.0, 1.4, 0.9],
         mean=0.5, seed=127, offset=0.5, gain=0.8),
]
TRAJECTORY = dict(case="logit_matern52_300x3", steps=10, learning_rate=0.05)

BERNOULLI_F = [-12.0, -9.5, -7.0, -5.0, -3.0, -2.0, -1.0, -0.5, -0.1, -1.0e-3, 0.0, 1.0e-3, 0.1, 0.5, 1.0, 2.0, 3.0, 5.0, 7.0, 9.5, 12.0]
POISSON_F = [-20.0, -12.0, -6.0, -3.0, -1.0, 0.0, 0.5, 1.0, 2.5, 4.0, 6.9, 9.2, 10.0]
POISSON_Y = [0.0, 1.0, 3.0, 17.0, 1000.0, 10000.0]


def pointwise():
    out = {}
    mp.mp.dps = 40
    for lik in ("probit", "logit", "poisson"):
        if lik == "poisson":
            f = np.repeat(POISSON_F, len(POISSON_Y))
            y = np.tile(POISSON_Y, len(POISSON_F))
        else:
            f = np.repeat(BERNOULLI_F, 2)
            y = np.tile([0.0, 1.0], len(BERNOULLI_F))
        gold = lo.derivs_mp(lik, f, y, dps=40)
        plain = lo.derivs64(lik, f, y)
        out["pw_%s_f" % lik], out["pw_%s_y" % lik] = f, y
        for name, g, p in zip(("lp", "d1", "W", "d3"), gold, plain):
            out["pw_%s_%s" % (lik, name)] = np.array([float(v) for v in g])
            out["pw_%s_%s_e64" % (lik, name)] = np.array([float(abs(mp.mpf(float(pv)) - gv)) for pv, gv in zip(p, g)])
        print("pointwise %-8s %d points" % (lik, f.size))
    return out


def model_case(case):
    inp = lo.case_inputs(case)
    o64 = lo.build_oracle(case, inp).search()
    old = lo.build_oracle(case, inp, dtype=lo.LD).search(until_stall=True)
    assert o64.steps <= 20, (case["name"], o64.steps)
    res = {"steps": o64.steps, "halvings": o64.halvings, "steps_ld": old.steps, "max_count": float(inp["y"].max())}
    e64 = {"loss": xr.rel_err(o64.loss(), old.loss())}
    res["loss"] = float(old.loss())
    g64, gld = o64.loss_grads(), old.loss_grads()
    names = ["variance", "length_scales"] + (["mean"] if case["mean"] is not None else [])
    e64["grad"] = max(xr.rel_err(a, b) for a, b, _ in zip(g64, gld, names))
    for nm, g in zip(names, gld):
        res["grad_" + nm] = np.asarray(g, dtype=np.float64)
    m64, v64 = o64.predict_f(inp["xs"])
    mld, vld = old.predict_f(inp["xs"])
    _, c64 = o64.predict_f(inp["xs"], diag=False)
    _, cld = old.predict_f(inp["xs"], diag=False)
    e64["mean"], e64["var"], e64["cov"] = xr.abs_err(m64, mld), xr.abs_err(v64, vld), xr.abs_err(c64, cld)
    res["mean"], res["var"], res["cov"] = (np.asarray(t, dtype=np.float64) for t in (mld, vld, cld))
    res["e64"] = e64
    print("%-28s loss %.10f steps %d (ld %d) halvings %d max count %g e64 %s" % (case["name"], res["loss"], o64.steps, old.steps, o64.halvings,
                                                                             res["max_count"], {k: "%.1e" % v for k, v in e64.items()}))
    return res


def trajectory(case):
    """torch's Adam (CPU, fp64) on the raw parameters of the fp64 statement: log variance, log length_scales, mean."""
    inp = lo.case_inputs(case)
    raw = [torch.tensor(np.log(np.atleast_1d(np.float64(case["variance"])))), torch.tensor(np.log(np.asarray(case["length_scales"], dtype=np.float64)))]
    if case["mean"] is not None:
        raw.append(torch.tensor([float(case["mean"])], dtype=torch.float64))
    opt = torch.optim.Adam(raw, lr=TRAJECTORY["learning_rate"])
    losses = []
    for _ in range(TRAJECTORY["steps"]):
        c = dict(case, variance=float(raw[0].exp()[0]), length_scales=raw[1].exp().numpy().copy(), mean=None if case["mean"] is None else float(raw[2][0]))
        o = lo.build_oracle(c, inp).search()
        losses.append(float(o.loss()))
        for p, g in zip(raw, o.loss_grads()):
            p.grad = torch.tensor(np.asarray(g, dtype=np.float64)).reshape(p.shape)
        opt.step()
    print("trajectory on %s: %s" % (case["name"], losses))
    return losses


def main():
    out = pointwise()
    meta = {"cases": [], "trajectory": dict(TRAJECTORY)}
    halved = False
    for case in CASES:
        res = model_case(case)
        halved |= case["lik"] == "poisson" and res["halvings"] >= 1
        entry = dict(case)
        for k, v in res.items():
            if isinstance(v, np.ndarray):
                out["%s__%s" % (case["name"], k)] = v
            else:
                entry[k] = v
        meta["cases"].append(entry)
    assert halved, "no Poisson case made the oracle halve a step"
    meta["trajectory"]["losses"] = trajectory(next(c for c in CASES if c["name"] == TRAJECTORY["case"]))
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "laplace_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
