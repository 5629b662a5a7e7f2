"""Goldens of EPGP (gptorch_amd/models/ep.py, csrc/ep.hip) -> tests/golden/ep_cases.npz.  CPU only:

    python tests/golden/make_ep_golden.py

(a) Pointwise: what gpn_ep_sites computes (tests/_ep_oracle.SITE_KEYS: the damped sites, log Z^, mu_hat, s2_hat, the site part of
    the evidence, the undamped changes) from its DEFINITIONS in 40-digit arithmetic (tests/_ep_oracle.sites_mp) over a grid of
    cavity mean in [-35, 35] x cavity variance in [1e-12, 1e6] x label x {empty site, a site of half the cavity's precision}, the
    prior mean alternating between 0 and 0.3, for both links (logit: the 20-node rule); beside each number the error e64 of the
    oracle's plain-fp64 closed form (sites64).  For the logit link e64 is the LARGEST error among sites64's LOGIT_VARIANTS orders
    of the sums over the nodes: at a small cavity variance 1 / s2_hat - tau_c cancels (by 1 / (tau v_c)), the error of one fp64
    evaluation is then a draw from a wide distribution, and a single draw that happens to be small would understate what fp64
    can do there.  The kernel's inputs (mu, sigma2, tau, nu) are stored: the goldens are functions of exactly those fp64 numbers.
(b) Model cases (tests/_ep_oracle.EPOracle: dense K; inputs from gptorch_amd.rng): the long-double loss (swept until the change
    stops shrinking), its gradients w.r.t. every raw parameter and the mean, predict_f mean / variance at 40 points, predict_y (the
    package's predict_mean_variance of those marginals), and for each the distance e64 of the plain-fp64 statement under the
    default stopping rule; the fp64 statement's sweep count.
(c) Three steps of torch's CPU Adam on the fp64 statement of one case.

The generator asserts that no case stalls or needs more than 60 sweeps under the default rule.
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

from tests import _ep_oracle as eo  # noqa: E402
from tests import _laplace_oracle as lo  # noqa: E402
from tests import _xref as xr  # noqa: E402

CASES = [
    dict(name="probit_rbf_300x2", lik="probit", kind="Rbf", n=300, d=2, ARD=False, variance=1.7, length_scales=[0.9], mean=None, seed=211, H=20),
    dict(name="probit_matern52_ard_513x3", lik="probit", kind="Matern52", n=513, d=3, ARD=True, variance=6.0, length_scales=[1.4, 1.0, 1.8],
         mean=0.3, seed=223, H=20),
    dict(name="logit_matern52_300x3", lik="logit", kind="Matern52", n=300, d=3, ARD=False, variance=2.5, length_scales=[1.1], mean=-0.2, seed=227,
         H=32),
    # a prior variance of 25 at a short length-scale: undamped parallel EP does not converge here
    dict(name="probit_rbf_var25_300x2", lik="probit", kind="Rbf", n=300, d=2, ARD=False, variance=25.0, length_scales=[0.5], mean=None, seed=11,
         H=20),
]
TRAJECTORY = dict(case="logit_matern52_300x3", steps=3, learning_rate=0.05)
DAMPING = 0.8
MAX_SWEEPS_SEEN = 60

GRID_MEAN = [-35.0, -20.0, -8.0, -3.0, -1.6, -1.4, -0.3, 0.0, 0.7, 2.0, 6.0, 15.0, 35.0]
GRID_VAR = [1.0e-12, 1.0e-6, 1.0e-2, 1.0, 30.0, 1.0e3, 1.0e6]
GRID_H = 20
GRID_DPS = 330      # exp(-35^2 / 2) = 1e-266 is subtracted from 1 in the definitions


def pointwise():
    out = {}
    mu_c, v_c, y, full = (a.ravel() for a in np.meshgrid(GRID_MEAN, GRID_VAR, [0.0, 1.0], [0.0, 1.0], indexing="ij"))
    tau_c, nu_c = 1.0 / v_c, mu_c / v_c
    tau, nu = full * 0.5 * tau_c, full * -0.3 * nu_c
    sigma2 = 1.0 / (tau_c + tau)
    mu = sigma2 * (nu_c + nu)
    m = np.where(np.arange(mu.size) % 2 == 0, 0.0, 0.3)
    for lik in ("probit", "logit"):
        gold = eo.sites_mp(lik, y, m, mu, sigma2, tau, nu, DAMPING, GRID_H, dps=GRID_DPS)
        plains = [eo.sites64(lik, y, m, mu, sigma2, tau, nu, DAMPING, GRID_H, variant=v) for v in range(eo.LOGIT_VARIANTS if lik == "logit" else 1)]
        for name, v in (("y", y), ("m", m), ("mu", mu), ("sigma2", sigma2), ("tau", tau), ("nu", nu)):
            out["pw_%s_%s" % (lik, name)] = v
        worst = {}
        for key in eo.SITE_KEYS:
            g = gold[key]
            out["pw_%s_%s" % (lik, key)] = np.array([float(v) for v in g])
            e = np.max([[float(abs(mp.mpf(float(pv)) - gv)) for pv, gv in zip(plain[key], g)] for plain in plains], 0)
            out["pw_%s_%s_e64" % (lik, key)] = e
            worst[key] = int(np.sum(e > 64.0 * 2.0 ** -53 * np.abs(out["pw_%s_%s" % (lik, key)])))
            assert all(np.all(np.isfinite(plain[key])) for plain in plains), (lik, key)
        assert min(float(v) for v in gold["s2_hat"]) > 0 and all(float(np.min(plain["s2_hat"])) > 0 for plain in plains)
        print("pointwise %-7s %d points; entries whose e64 exceeds 64 ulp of the golden: %s" % (lik, mu.size, worst))
    return out


def predict_y(case, mean, var):
    from gptorch_amd import likelihoods
    lik = likelihoods.Bernoulli(case["lik"])
    lik.num_gauss_hermite_points = int(case["H"])
    pm, pv = lik.predict_mean_variance(torch.tensor(np.asarray(mean, dtype=np.float64))[:, None], torch.tensor(np.asarray(var, dtype=np.float64))[:, None])
    return pm[:, 0].numpy(), pv[:, 0].numpy()


def model_case(case):
    inp = lo.case_inputs(case)
    o64 = eo.build_oracle(case, inp).search(damping=DAMPING)
    old = eo.build_oracle(case, inp, dtype=eo.LD).search(damping=DAMPING, until_stall=True)
    assert not o64.stalled and o64.sweeps <= MAX_SWEEPS_SEEN, (case["name"], o64.sweeps, o64.stalled)
    res = {"sweeps": o64.sweeps, "sweeps_ld": old.sweeps, "loss": float(old.loss())}
    e64 = {"loss": xr.rel_err(o64.loss(), old.loss())}
    g64, gld = o64.loss_grads(), old.loss_grads()
    names = ["variance", "length_scales"] + (["mean"] if case["mean"] is not None else [])
    e64["grad"] = max(xr.rel_err(a, b) for a, b, _ in zip(g64, gld, names))
    for nm, g in zip(names, gld):
        res["grad_" + nm] = np.asarray(g, dtype=np.float64)
    m64, v64 = o64.predict_f(inp["xs"])
    mld, vld = old.predict_f(inp["xs"])
    e64["mean"], e64["var"] = xr.abs_err(m64, mld), xr.abs_err(v64, vld)
    res["mean"], res["var"] = np.asarray(mld, dtype=np.float64), np.asarray(vld, dtype=np.float64)
    res["py_mean"], res["py_var"] = predict_y(case, res["mean"], res["var"])
    res["e64"] = e64
    res["laplace_loss"] = float(lo.build_oracle(case, inp).search().loss())
    print("%-28s loss %.10f (Laplace %.6f) sweeps %d (ld %d) e64 %s" % (case["name"], res["loss"], res["laplace_loss"], o64.sweeps, old.sweeps,
                                                                       {k: "%.1e" % v for k, v in e64.items()}))
    return res


def trajectory(case):
    """torch's Adam (CPU, fp64) on the raw parameters of the fp64 statement: log variance, log length_scales, mean; every
    evaluation starts at the sites of the one before, as the model's warm start does."""
    inp = lo.case_inputs(case)
    raw = [torch.tensor(np.log(np.atleast_1d(np.float64(case["variance"])))), torch.tensor(np.log(np.asarray(case["length_scales"], dtype=np.float64)))]
    if case["mean"] is not None:
        raw.append(torch.tensor([float(case["mean"])], dtype=torch.float64))
    opt = torch.optim.Adam(raw, lr=TRAJECTORY["learning_rate"])
    losses, sites = [], None
    for _ in range(TRAJECTORY["steps"]):
        c = dict(case, variance=float(raw[0].exp()[0]), length_scales=raw[1].exp().numpy().copy(), mean=None if case["mean"] is None else float(raw[2][0]))
        o = eo.build_oracle(c, inp).search(sites0=sites, damping=DAMPING)
        sites = (o.tau, o.nu)
        losses.append(float(o.loss()))
        for p, g in zip(raw, o.loss_grads()):
            p.grad = torch.tensor(np.asarray(g, dtype=np.float64)).reshape(p.shape)
        opt.step()
    print("trajectory on %s: %s" % (case["name"], losses))
    return losses


def main():
    out = pointwise()
    meta = {"cases": [], "trajectory": dict(TRAJECTORY), "damping": DAMPING, "grid_H": GRID_H}
    for case in CASES:
        res = model_case(case)
        entry = dict(case)
        for k, v in res.items():
            if isinstance(v, np.ndarray):
                out["%s__%s" % (case["name"], k)] = v
            else:
                entry[k] = v
        meta["cases"].append(entry)
    meta["trajectory"]["losses"] = trajectory(next(c for c in CASES if c["name"] == TRAJECTORY["case"]))
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ep_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
