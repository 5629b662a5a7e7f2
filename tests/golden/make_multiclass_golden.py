"""Goldens of likelihoods.MultiClass (csrc/multiclass.hip) -> tests/golden/multiclass_cases.npz.  CPU only, a few minutes:

    python tests/golden/make_multiclass_golden.py

(a) Pointwise: per-row value, g_mean, g_var and the class probabilities of the robust-max rule from its DEFINITION in 40-digit
    arithmetic (tests/_multiclass_oracle.row_mp / probs_mp) at the oracle's golden points -- C in {2, 3, 10, 65} x H in
    {1, 20, 64}, gaps (mu_y - mu_c) / sqrt(v) out to +-40, ties, v in {1e-12, 1e-3, 1, 1e3} -- and beside each number e64, the
    largest error among the oracle's plain-fp64 evaluations (rows64 / probs64, VARIANTS orders and associations).  The inputs
    are regenerated from the oracle's point(); they are stored too, and the tests compare them.
(b) C = 2, H = 64: the largest distance of the rule's P from its closed form Phi((mu_y - mu_o) / sqrt(2 v)) over the gaps
    -6, -5.5 .. 6 (in 40 digits): the accuracy of the 64-node rule on that grid.
(c) Model cases (SVGP, N = 300, d = 2, M = 20, C in {3, 5}; full batch and the 64 rows drawn after np.random.seed(11)): the
    marginals of tests/_svgp_oracle's fp64 statement, the data term and its gradients w.r.t. the marginals in 40 digits, and
    e64 of the plain-fp64 evaluation of the same: relative to max(1, |.|) as tests/_xref.rel_err; the class probabilities at 16
    new points with their e64.
(d) Three well-separated blobs: the generator ASSERTS that 200 Adam steps of the torch route on the CPU (from q_mu = 0,
    S_L = I) reach a training accuracy of 1.0, and stores the losses' ends.
"""
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _multiclass_oracle as mo  # noqa: E402


def _point_job(args):
    mu, v, label, H = args
    val, gm, gv, _ = mo.row_mp(mu, v, label, mo.EPS, H)
    pr = mo.probs_mp(mu, v, mo.EPS, H)
    plains = [mo.rows64(mu[None], np.array([v]), np.array([label]), mo.EPS, H, k) for k in range(mo.VARIANTS)]
    pplains = [mo.probs64(mu[None], np.array([v]), mo.EPS, H, k) for k in range(mo.VARIANTS)]
    return dict(val=float(val), gm=[float(g) for g in gm], gv=float(gv), probs=[float(p) for p in pr],
                val_e64=mo.worst_e64([p[0] for p in plains], [val])[0], gm_e64=mo.worst_e64([p[1] for p in plains], gm),
                gv_e64=mo.worst_e64([p[2] for p in plains], [gv])[0], probs_e64=mo.worst_e64(pplains, pr))


def pointwise(pool):
    out = {}
    for C in mo.CLASSES:
        mu, v, lab = mo.points(C)
        out["C%d_mu" % C], out["C%d_v" % C], out["C%d_label" % C] = mu, v, lab
        for H in mo.HS:
            res = pool.map(_point_job, [(mu[p], v[p], lab[p], H) for p in range(len(v))])
            for key in ("val", "gm", "gv", "probs", "val_e64", "gm_e64", "gv_e64", "probs_e64"):
                out["C%d_H%d_%s" % (C, H, key)] = np.array([r[key] for r in res], dtype=np.float64)
            U = 2.0 ** -53
            over = {k: int(np.sum(out["C%d_H%d_%s_e64" % (C, H, k)] > 64.0 * U * np.abs(out["C%d_H%d_%s" % (C, H, k)])))
                    for k in ("val", "gm", "gv", "probs")}
            print("C=%d H=%d: %d points; entries whose e64 exceeds 64 ulp of the golden: %s" % (C, H, len(v), over), flush=True)
    return out


def rule_accuracy_c2():
    import mpmath as mp
    worst = mp.mpf(0)
    with mp.workdps(mo.DPS):
        for g in np.arange(-6.0, 6.01, 0.5):
            P = mo.row_mp(np.array([float(g), 0.0]), 1.0, 0.0, mo.EPS, 64)[3]
            worst = max(worst, abs(P - mp.ncdf(mp.mpf(float(g)) / mp.sqrt(2))))
    return float(worst)


def _rows_job(args):
    mu, v, label, H = args
    val, gm, gv, _ = mo.row_mp(mu, v, label, mo.EPS, H)
    return float(val), [float(g) for g in gm], float(gv)


def model_case(pool, case):
    import torch
    inp = mo.model_inputs(case)
    C, H = case["C"], case["H"]
    o = mo.svgp_oracle(inp, C, mo.EPS, H, case["variance"], case["length_scale"], q_mu=inp["q_mu"], q_sqrt=inp["q_sqrt"])
    res, arrays = {}, {}
    for tag, nb in (("full", None), ("batch64", 64)):
        idx = mo.batch_indices(case, nb)
        with torch.no_grad():
            mean, var = o.marginals(o.X[idx])
        mean, var, lab = mean.numpy(), var.numpy(), inp["y"][idx, 0]
        gold = pool.map(_rows_job, [(mean[i], var[i], lab[i], H) for i in range(len(idx))])
        scale = case["n"] / len(idx)
        term = scale * float(np.sum(np.array([g[0] for g in gold], dtype=np.longdouble)))
        gm, gv = np.array([g[1] for g in gold]), np.array([g[2] for g in gold])
        e_loss, e_grad = 0.0, 0.0
        for k in range(mo.VARIANTS):
            v64, gm64, gv64 = mo.rows64(mean, var, lab, mo.EPS, H, k)
            e_loss = max(e_loss, abs(scale * float(np.sum(v64.astype(np.longdouble))) - term) / max(1.0, abs(term)))
            e_grad = max(e_grad, float(np.max(np.abs(gm64 - gm))) / max(1.0, float(np.max(np.abs(gm)))),
                         float(np.max(np.abs(gv64 - gv))) / max(1.0, float(np.max(np.abs(gv)))))
        res[tag] = dict(data_term=term, e64_loss=e_loss, e64_grad=e_grad, loss=float(o.loss(idx=idx).item()))
        print("%s %-7s data term %.12f loss %.12f e64 loss %.1e grad %.1e" % (case["name"], tag, term, res[tag]["loss"], e_loss, e_grad), flush=True)
    fm, fv = o.predict_f(inp["xs"])
    pr = pool.starmap(mo.probs_mp, [(fm[i], fv[i], mo.EPS, H) for i in range(fm.shape[0])])
    probs = np.array([[float(p) for p in row] for row in pr])
    res["e64_mean"] = max(float(np.max(np.abs(mo.probs64(fm, fv, mo.EPS, H, k) - probs))) for k in range(mo.VARIANTS))
    arrays["%s__probs" % case["name"]] = probs
    print("%s predict_y e64 %.1e, rows add to 1 within %.1e" % (case["name"], res["e64_mean"], float(np.max(np.abs(probs.sum(1) - 1.0)))), flush=True)
    return res, arrays


def blobs():
    import torch
    inp = mo.blob_inputs()
    b = mo.BLOBS
    o = mo.svgp_oracle(inp, b["C"], mo.EPS, b["H"], 1.0, 1.0)
    losses = o.optimize_adam(b["steps"], learning_rate=b["learning_rate"])
    mean, _ = o.predict_f(inp["x"])
    acc = float(np.mean(np.argmax(mean, 1) == inp["y"][:, 0]))
    print("blobs: loss %.4f -> %.4f, training accuracy %.3f" % (losses[0], losses[-1], acc), flush=True)
    assert acc == 1.0, acc
    return dict(first_loss=losses[0], last_loss=losses[-1], accuracy=acc)


def main():
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        out = pointwise(pool)
        meta = {"eps": mo.EPS, "c2_h64_rule_accuracy": rule_accuracy_c2(), "cases": {}}
        print("C = 2, H = 64: the rule's P within %.2e of Phi(gap / sqrt 2)" % meta["c2_h64_rule_accuracy"], flush=True)
        for case in mo.MODEL_CASES:
            res, arrays = model_case(pool, case)
            meta["cases"][case["name"]] = res
            out.update(arrays)
    meta["blobs"] = blobs()
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "multiclass_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
