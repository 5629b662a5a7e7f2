#!/usr/bin/env python3
"""GPU-box tool: what the closed-form k-fold objective of GPR costs on one MI355X, beside the leave-one-out objective and the log
marginal likelihood of the SAME model in the same process, and beside the status-quo way to a k-fold score (k refitted models).

Matern52, d = 8, dy = 1, N in {2048, 8192}, k in {5, 10} (contiguous folds).  Per (N, k), interleaved round by round (host clock
around work that ends in a device synchronise; medians, minima, maxima):

    kfold_loss_backward   loss(); backward() with objective="kfold": factorisation, U = L^-T, P = U U^T, a, the k fold blocks
                          gathered and factorised in lock step, q, w; then P[:, I_f], S, Q = S S^T, the gradient sweep
    loo_loss_backward     loss(); backward() with objective="loo" on the same data and hyper-parameters
    lml_loss_backward     ... with objective="lml": the yardstick (flop model: k-fold = (2 + 2 / k) x this)
    kfold_score           kfold_log_predictive() under no_grad
    refit_score           the same score the status-quo way (unchanged code): k GPR models on the k training subsets (built once,
                          outside the clock), batched_factorise, predict_y(diag=False) on each held-out fold, the multivariate
                          normal log density in torch

and score_abs_diff = |kfold_score - refit_score| (the two routes agree to rounding or something is wrong).

    python tools/kfold_bench.py [--sizes 2048,8192] [--folds 5,10] [--rounds 9] [--warmup 2] [--out profiles/kfold_step.json]
                                [--markdown FILE]   (FILE: the table of the LAB.md section, from the same numbers)
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from gptorch_amd import kernels, likelihoods, rng  # noqa: E402
from gptorch_amd.models import GPR, batched_factorise  # noqa: E402


def stats(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts))}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(s):
    return "%.1f [%.1f, %.1f]" % (s["ms_median"], s["ms_min"], s["ms_max"])


def markdown(result):
    lines = ["| N | k | k-fold step ms | LOO step ms | LML step ms | k-fold / LML (model) | LOO / LML | k-fold score ms | k refits score ms | refits / closed form | score abs diff |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in result["rows"]:
        lines.append("| %d | %d | %s | %s | %s | %.2f (%.2f) | %.2f | %s | %s | %.2f | %.1e |" % (
            r["n"], r["k"], fmt(r["kfold_loss_backward"]), fmt(r["loo_loss_backward"]), fmt(r["lml_loss_backward"]),
            r["ratio_kfold_lml"], r["ratio_model"], r["ratio_loo_lml"], fmt(r["kfold_score"]), fmt(r["refit_score"]),
            r["ratio_refit_closed"], r["score_abs_diff"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,8192")
    ap.add_argument("--folds", default="5,10")
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kfold_bench.py measures on the GPU; there is none here")
    d = args.d
    result = {"workload": "GPR Matern52 d=%d dy=1 fp64, objective=\"kfold\" (contiguous folds) beside \"loo\" and \"lml\" on the same points and "
                          "hyper-parameters, and beside k refitted models (batched_factorise + predict_y(diag=False) + MVN log density), one "
                          "MI355X, legs interleaved round by round, host clock around a device synchronise" % d, "rows": []}

    def write():
        for path, text in ((args.out, json.dumps(result, indent=1)), (args.markdown, markdown(result))):
            if path:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, "w") as fh:
                    fh.write(text)

    for n in (int(v) for v in args.sizes.split(",")):
        x, y = rng.make_regression(n, d, 1, seed=0)
        for k in (int(v) for v in args.folds.split(",")):
            def model(objective, xs=x, ys=y, **kw):
                m = GPR(xs, ys, kernels.Matern52(d, variance=1.0, length_scales=float(np.sqrt(d))), likelihood=likelihoods.Gaussian(variance=0.05),
                        objective=objective, **kw)
                m.cuda()
                return m
            kf, loo, lml = model("kfold", folds=k), model("loo"), model("lml")
            held = np.array_split(np.arange(n), k)
            refits = [model("lml", np.delete(x, te, 0), np.delete(y, te, 0)) for te in held]
            tests = [(torch.tensor(x[te]).cuda(), torch.tensor(y[te]).cuda()) for te in held]

            def kfold_score():
                with torch.no_grad():
                    return kf.kfold_log_predictive()

            def refit_score():
                with torch.no_grad():
                    for m in refits:
                        m._predict_cache = None          # a score starts without factors: no round reuses the one before
                    batched_factorise(refits)
                    total = torch.zeros((), dtype=torch.float64, device="cuda")
                    for m, (xt, yt) in zip(refits, tests):
                        mean, cov = m.predict_y(xt, diag=False)
                        L = torch.linalg.cholesky(cov)
                        z = torch.linalg.solve_triangular(L, yt - mean, upper=False)
                        total = total - 0.5 * (z * z).sum() - L.diagonal().log().sum() - 0.5 * xt.shape[0] * math.log(2 * math.pi)
                    return total

            def loss_backward(m):
                def run():
                    m.zero_grad()
                    loss = m.loss()
                    loss.backward()
                    return loss
                return run

            legs = {"kfold_loss_backward": loss_backward(kf), "loo_loss_backward": loss_backward(loo), "lml_loss_backward": loss_backward(lml),
                    "kfold_score": kfold_score, "refit_score": refit_score}
            ts = {name: [] for name in legs}
            last = {}
            for r in range(args.rounds + args.warmup):
                for name, fn in legs.items():
                    t, out = timed(fn)
                    last[name] = out
                    if r >= args.warmup:
                        ts[name].append(t)
            row = {"n": n, "k": k, "d": d, "rounds": args.rounds, "warmup": args.warmup}
            row.update({name: stats(v) for name, v in ts.items()})
            med = lambda name: row[name]["ms_median"]
            row["ratio_kfold_lml"] = med("kfold_loss_backward") / med("lml_loss_backward")
            row["ratio_loo_lml"] = med("loo_loss_backward") / med("lml_loss_backward")
            row["ratio_model"] = 2.0 + 2.0 / k
            row["ratio_refit_closed"] = med("refit_score") / med("kfold_score")
            row["kfold_score_value"] = float(last["kfold_score"].item())
            row["refit_score_value"] = float(last["refit_score"].item())
            row["score_abs_diff"] = abs(row["kfold_score_value"] - row["refit_score_value"])
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
            write()
            del kf, loo, lml, refits, tests, legs, last
            torch.cuda.empty_cache()
    write()


if __name__ == "__main__":
    main()
