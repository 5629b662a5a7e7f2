"""
Generator of the SVGP fixtures (run on the CPU, in the build environment that has the reference checked out read-only):

  ref_svgp_fixtures.npz   the reference's own SVGP data files (test/data/models/sparse_gpr: q_mu, l_s, svgp_y_mean,
                          svgp_y_cov) and the value its loss evaluates to today next to the pinned 9.534628739243518
                          (test/test_models/test_sparse_gpr.py:220)
  svgp_cases.json/.npz    bound, raw-parameter gradients (the reference's autograd) and predictions of the cases below, a
                          20-step minibatch Adam trajectory, and the reference's _init_posterior values under a seed

Every value written comes from the reference (gptorch/models/sparse_gpr.py:198-381); tests/_svgp_oracle.py is asserted to
agree with it at least ten times tighter than the tolerance the GPU tests use (bound 1e-9 relative -- 1e-9 absolute on the
well-conditioned case --, predictions 1e-9, gradients 1e-8 x max|reference gradient| per block, trajectory 1e-9).
The well-conditioned case (inducing points = k-means centres, stored; cond K(Z) recorded) is held to 1e-8 ABSOLUTE: its noise
variance (0.1) and the 0.5-scale induced_output_mean keep |bound| near 1e5, where 1e-8 is ~700 ulp -- room for the rounding
of two differently ordered fp64 sums over 16384 terms (~sqrt(N) ulp typical), which 1e-2 noise (|bound| ~ 1e6) would not leave.
Only data is written; the reference never travels to the GPU box.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import gptorch  # noqa: E402  (the reference)

assert gptorch.__file__.startswith(REF), gptorch.__file__
from gptorch import kernels as rk, likelihoods as rl, mean_functions as rm  # noqa: E402,F401
from gptorch.models.sparse_gpr import SVGP as RefSVGP  # noqa: E402

gptorch.models.SVGP = RefSVGP
from gptorch_amd import rng  # noqa: E402
from tests import _svgp_oracle as so  # noqa: E402


def tril_pack(a):
    a = np.asarray(a)
    return a[np.tril_indices(a.shape[0])]


def check(what, got, want, tol, scale=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    s = max(1.0, float(np.max(np.abs(want)))) if scale is None else scale
    err = float(np.max(np.abs(got - want))) / s
    assert err < tol, "%s: oracle vs reference %.3e (allowed %.1e)" % (what, err, tol)
    return err


def ref_eval(case, inp, idx):
    """loss and raw-parameter gradients of the reference on all data (idx None) or on the rows idx."""
    m = so.build_model(gptorch, case, inp)
    m.zero_grad()
    if idx is None:
        loss = m.loss()
    else:
        loss = m.loss(x=m.X[idx], y=m.Y[idx])
    loss.backward()
    return loss.item(), {n: p.grad.numpy().copy() for n, p in m.named_parameters() if p.grad is not None}


def gen_fixtures(out):
    ddir = os.path.join(REF, "test", "data", "models", "sparse_gpr")
    load = lambda k: np.atleast_2d(np.loadtxt(os.path.join(ddir, k + ".dat")))
    pack = {k: load(k) for k in ["q_mu", "l_s", "svgp_y_mean", "svgp_y_cov"]}
    base = {k: load(k) for k in ["x", "y", "z", "x_test"]}
    for d in (pack, base):
        for k in ["q_mu", "svgp_y_mean", "x", "y", "z", "x_test"]:
            if k in d and d[k].shape[0] == 1:
                d[k] = d[k].T
    kern = rk.Matern32(1)
    kern.length_scales.data = torch.zeros(1, dtype=torch.float64)
    kern.variance.data = torch.zeros(1, dtype=torch.float64)
    np.random.seed(0)
    m = RefSVGP(base["x"], base["y"], kern, inducing_points=base["z"], likelihood=rl.Gaussian(variance=1.0), mean_function=rm.Zero(1))
    m.induced_output_mean.data = torch.tensor(pack["q_mu"])
    m.induced_output_chol_cov.data = m.induced_output_chol_cov._transform.inv(torch.tensor(pack["l_s"]))
    loss = m.loss().item()
    pin = 9.534628739243518
    pack["svgp_loss_reference_run"] = np.array([loss])
    pack["svgp_loss_pinned"] = np.array([pin])
    pack["reference_run_within_approx_of_pin"] = np.array([abs(loss - pin) < 1e-6 * pin])
    o = so.SVGPOracle(base["x"], base["y"], base["z"], dict(kind="Matern32", variance=1.0, length_scales=1.0), noise=1.0,
                      q_mu=pack["q_mu"], q_sqrt=pack["l_s"])
    assert abs(o.loss().item() - loss) < 1e-10, (o.loss().item(), loss)
    mu, s = m._predict(torch.tensor(base["x_test"]), diag=False)
    assert np.allclose(mu.detach().numpy().ravel(), pack["svgp_y_mean"].ravel()) and np.allclose(s.detach().numpy(), pack["svgp_y_cov"])
    omu, ocov = o.predict_f(base["x_test"], diag=False)
    check("fixture mean", omu.ravel(), pack["svgp_y_mean"].ravel(), 1e-9)
    check("fixture cov", ocov, pack["svgp_y_cov"], 1e-9)
    np.savez(os.path.join(out, "ref_svgp_fixtures.npz"), **pack)
    print("fixtures: reference loss today %.15f (pinned %.15f, |diff| %.2e)" % (loss, pin, abs(loss - pin)))


def gen_case(case, arrays, z=None):
    """fills case["evals"] (all data and, with nb, the explicit index set) and the predictions; big arrays -> `arrays`."""
    inp = so.case_inputs(case, z=z)
    names = so.model_names(case)
    case["evals"] = []
    for tag, idx in [("full", None)] + ([("batch", inp["idx"])] if inp["idx"] is not None else []):
        loss, grads = ref_eval(case, inp, idx)
        o = so.oracle_for(case, inp)
        oloss, ograds = o.loss_and_grads(idx=idx)
        ev = dict(tag=tag, loss=loss)
        if case.get("absolute"):
            ev["oracle_abs_diff"] = abs(oloss - loss)
            assert ev["oracle_abs_diff"] < 1e-9, ev["oracle_abs_diff"]
        ev["oracle_rel_diff"] = check(case["name"] + " bound", oloss, loss, 1e-9, scale=abs(loss))
        ev["grads"] = {}
        for on, mn in names.items():
            g = grads[mn]
            check("%s %s d/d%s" % (case["name"], tag, mn), ograds[on].reshape(g.shape), g, 1e-8, scale=float(np.max(np.abs(g))))
            if g.size > 64:
                key = "%s.%s.%s" % (case["name"], tag, mn)
                arrays[key] = tril_pack(g) if mn == "induced_output_chol_cov" else g
                ev["grads"][mn] = "npz:" + key
            else:
                ev["grads"][mn] = g.tolist()
        case["evals"].append(ev)
    m = so.build_model(gptorch, case, inp)
    with torch.no_grad():
        xs = torch.tensor(inp["xs"])
        mu, var = m._predict(xs)
        _, cov = m._predict(xs, diag=False)
    o = so.oracle_for(case, inp)
    omu, ovar = o.predict_f(inp["xs"])
    _, ocov = o.predict_f(inp["xs"], diag=False)
    check(case["name"] + " mean", omu, mu.numpy(), 1e-9, scale=1.0)
    check(case["name"] + " var", ovar, var.numpy()[:, 0], 1e-9, scale=1.0)
    check(case["name"] + " cov", ocov, cov.numpy(), 1e-9, scale=1.0)
    case.update(mean_pred=mu.tolist(), var_pred=var[:, 0].tolist(), cov_pred=cov.tolist())
    print("%s: loss %.10f (oracle rel %.1e)" % (case["name"], case["evals"][0]["loss"], case["evals"][0]["oracle_rel_diff"]))
    return case


def gen_trajectory(steps=20):
    case = dict(name="adam_matern52_2000_64_b256", n=2000, d=3, dy=1, m=64, kernel=dict(kind="Matern52", variance=1.1, length_scales=1.4),
                noise=0.1, seed_x=0, seed_z=91, seed_q=92, seed_xs=93, batch_size=256, np_seed=1234, steps=steps, learning_rate=0.01)
    inp = so.case_inputs(case)
    m = so.build_model(gptorch, case, inp, batch_size=case["batch_size"])
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=case["learning_rate"])   # base.py:150-151
    np.random.seed(case["np_seed"])
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = m.loss()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    o = so.oracle_for(case, inp, batch_size=case["batch_size"])
    np.random.seed(case["np_seed"])
    olosses = o.optimize_adam(steps, case["learning_rate"])
    check("trajectory losses", olosses, losses, 1e-9)
    final = {n: p.detach().numpy().copy() for n, p in m.named_parameters()}
    for on, mn in so.model_names(case).items():
        check("trajectory final " + mn, o.raw[on].detach().numpy().reshape(final[mn].shape), final[mn], 1e-9)
    case["losses"] = losses
    return case, final


def gen_init():
    """the reference's _init_posterior (sparse_gpr.py:310-335) under np.random.seed: the values a construction must give."""
    case = dict(name="init_matern52_const", n=400, d=2, dy=2, m=20, kernel=dict(kind="Matern52", variance=1.3, length_scales=1.2),
                noise=0.1, mean=[0.3, -0.2], seed_x=0, seed_z=95, seed_q=96, seed_xs=97, np_seed=7)
    inp = so.case_inputs(case)
    kern = rk.Matern52(case["d"], variance=1.3, length_scales=1.2)
    np.random.seed(case["np_seed"])
    m = RefSVGP(inp["x"], inp["y"], kern, inducing_points=inp["z"].copy(), likelihood=rl.Gaussian(variance=case["noise"]),
                mean_function=rm.Constant(2, val=torch.tensor(case["mean"], dtype=torch.float64)))
    case["next_draw"] = int(np.random.permutation(1000)[0])                 # the constructor consumed exactly one permutation
    case["induced_output_mean"] = m.induced_output_mean.detach().tolist()
    case["induced_output_chol_cov"] = m.induced_output_chol_cov.transform().detach().tolist()
    return case


def main(out=HERE):
    from scipy.cluster.vq import kmeans2
    gen_fixtures(out)
    arrays = {}
    well = dict(name="wellcond_matern52_8192_256_4", n=8192, d=4, dy=2, m=256, kernel=dict(kind="Matern52", variance=1.2, length_scales=1.0),
                noise=0.1, seed_x=0, seed_z=0, seed_q=81, seed_xs=82, nb=1000, seed_idx=83, absolute=True)
    x, _ = rng.make_regression(well["n"], well["d"], well["dy"], seed=well["seed_x"])
    z, _ = kmeans2(x, well["m"], minit="points", seed=1234, iter=20)
    arrays["wellcond.z"] = z
    Kuu = rk.Matern52(4, variance=1.2, length_scales=1.0).K(torch.tensor(z)).detach()
    ev = torch.linalg.eigvalsh(Kuu)
    well["cond_Kuu"] = float(ev[-1] / ev[0])
    torch.linalg.cholesky(Kuu)                                              # factors as it is: no ladder rung
    cases = [gen_case(well, arrays, z=z)]
    small = [
        dict(name="rbf_ard_300_24_3", n=300, d=3, dy=1, m=24, kernel=dict(kind="Rbf", variance=0.8, length_scales=[0.8, 1.0, 1.3], ARD=True),
             noise=0.1, seed_x=0, seed_z=61, seed_q=62, seed_xs=63, nb=100, seed_idx=64),
        dict(name="matern32_250_20_2", n=250, d=2, dy=2, m=20, kernel=dict(kind="Matern32", variance=1.4, length_scales=0.9),
             noise=0.2, seed_x=0, seed_z=65, seed_q=66, seed_xs=67),
        dict(name="exp_250_20_2", n=250, d=2, dy=1, m=20, kernel=dict(kind="Exp", variance=0.9, length_scales=1.5),
             noise=0.2, seed_x=0, seed_z=68, seed_q=69, seed_xs=70, nb=77, seed_idx=71),
        dict(name="matern52_const_mean_300_24_2", n=300, d=2, dy=2, m=24, kernel=dict(kind="Matern52", variance=1.1, length_scales=1.2),
             noise=0.1, mean=[0.4, -0.3], seed_x=0, seed_z=72, seed_q=73, seed_xs=74, nb=120, seed_idx=75),
        dict(name="linear_rbf_constant_300_24_2", n=300, d=2, dy=1, m=24,
             kernel=dict(kind="Linear+Rbf+Constant", linear_variance=0.5, variance=1.0, length_scales=1.1, constant=0.3),
             noise=0.1, seed_x=0, seed_z=76, seed_q=77, seed_xs=78, nb=100, seed_idx=79),
    ]
    cases += [gen_case(c, arrays) for c in small]
    traj, final = gen_trajectory()
    for n, v in final.items():
        arrays["trajectory.final." + n] = tril_pack(v) if n == "induced_output_chol_cov" else v
    init = gen_init()
    np.savez(os.path.join(out, "svgp_cases.npz"), **arrays)
    with open(os.path.join(out, "svgp_cases.json"), "w") as f:
        json.dump(dict(cases=cases, trajectory=traj, init=init), f, indent=1)
    print("wrote svgp_cases.json / .npz (cond K(Z) of the well-conditioned case: %.3e)" % well["cond_Kuu"])


if __name__ == "__main__":
    with contextlib.redirect_stdout(sys.stdout):
        main()
