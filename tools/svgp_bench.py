#!/usr/bin/env python3
"""GPU-box tool: one SVGP optimiser step's loss(); backward() on one MI355X -- the native node (models/sparse_gpr.py SVGP,
csrc/svgp.hip) against THE SAME bound composed from the public pieces that exist without it (kernel.K, functions.cholesky,
functions.trtrs, torch autograd on the GPU: the reference's op chain, sparse_gpr.py:263-381).  N = 1e6, d = 8, dy = 1,
Matern52; the two legs are interleaved step by step on the same pre-drawn minibatches; medians; one JSON line.

    python tools/svgp_bench.py [--shapes 1024x256,4096x1024,16384x2048] [--steps 20] [--warmup 3] [--out profiles/svgp_step.json]
    rocprofv3 --kernel-trace --stats -d DIR -o svgp --output-format csv -- python tools/svgp_bench.py --shapes 16384x2048 --native-only --steps 1 --warmup 2
    python tools/svgp_bench.py --fold-trace DIR/svgp_kernel_stats.csv --shapes 16384x2048 --steps 1 --warmup 2 --out profiles/svgp_step.json
"""
import argparse
import csv
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from gptorch_amd import functions, kernels, likelihoods, rng  # noqa: E402
from gptorch_amd.models import SVGP  # noqa: E402

HBM_PEAK = 8.0e12      # bytes/s, MI355X data sheet


def composed_loss(model, xb, yb):
    """the bound of sparse_gpr.py:263-308 from the public differentiable pieces (one autograd node per op)."""
    k, Z = model.kernel, model.Z
    m, dy = model.induced_output_mean.shape
    L = functions.cholesky(k.K(Z))
    alpha = functions.trtrs(k.K(Z, xb), L).t()
    S_L = model.induced_output_chol_cov.transform()
    beta = functions.trtrs(S_L, L)
    w = functions.trtrs(model.induced_output_mean, L)
    f_mean = alpha @ w
    gamma = alpha @ beta
    f_var = k.Kdiag(xb) - (alpha ** 2).sum(1) + (gamma ** 2).sum(1)
    s2 = model.likelihood.variance.transform()
    data = -0.5 * (yb.nelement() * (math.log(2.0 * math.pi) + torch.log(s2)) + (((yb - f_mean) ** 2).sum() + dy * f_var.sum()) / s2)
    kl = 0.5 * dy * ((beta ** 2).sum() - m + 2.0 * L.diagonal().log().sum() - 2.0 * S_L.diagonal().log().sum()) + 0.5 * (w ** 2).sum()
    return -(data.reshape(()) * (model.num_data / xb.shape[0]) - kl)


def fold_trace(path):
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {"launches": sum(int(r["Calls"]) for r in rows), "kernel_time_ms": total / 1e6, "kernels": []}
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        out["kernels"].append({"name": r["Name"][:100], "calls": int(r["Calls"]), "total_us": float(r["TotalDurationNs"]) / 1e3,
                               "share": float(r["TotalDurationNs"]) / total})
    out["row_kernel_share"] = sum(k["share"] for k in out["kernels"] if "svgp_" in k["name"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--shapes", default="1024x256,4096x1024,16384x2048")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--fold-trace", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    if args.fold_trace:
        nb, m = shapes[0]
        tr = fold_trace(args.fold_trace)
        for k in tr["kernels"]:                                           # achieved bytes/s of the two row kernels
            if "svgp_marginals" in k["name"]:
                k["bytes_per_s"] = 2.0 * nb * m * 8 * k["calls"] / (k["total_us"] * 1e-6)
            if "svgp_backward_rows" in k["name"]:
                k["bytes_per_s"] = 5.0 * nb * m * 8 * k["calls"] / (k["total_us"] * 1e-6)
            if "bytes_per_s" in k:
                k["frac_hbm_peak"] = k["bytes_per_s"] / HBM_PEAK
        result = {"trace_shape": [nb, m], "trace_steps": args.steps + args.warmup, "trace": tr}
        if args.out and os.path.exists(args.out):
            result = dict(json.load(open(args.out)), **result)
    else:
        n, d = args.n, args.d
        x, y = rng.make_regression(n, d, 1, seed=0)
        result = {"workload": "SVGP Matern52 N=%d d=%d dy=1 fp64, loss(); backward(), one MI355X" % (n, d), "shapes": []}
        for nb, m in shapes:
            z = rng.normal(99, (m, d))
            np.random.seed(0)
            model = SVGP(x[:4000], y[:4000], kernels.Matern52(d, variance=1.0, length_scales=float(np.sqrt(d))), inducing_points=z,
                         likelihood=likelihoods.Gaussian(variance=0.1), batch_size=nb)
            model.cuda()
            model.X, model.Y = torch.tensor(x).cuda(), torch.tensor(y).cuda()
            rs = np.random.RandomState(1)
            total = args.steps + args.warmup
            batches = [torch.as_tensor(rs.permutation(n)[:nb]).cuda() for _ in range(total)]

            def step(fn, i):
                xb, yb = model.X[batches[i]], model.Y[batches[i]]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.zero_grad()
                loss = fn(xb, yb)
                loss.backward()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, loss.item()
            native = lambda xb, yb: model.loss(x=xb, y=yb)
            composed = lambda xb, yb: composed_loss(model, xb, yb)
            tn, tc, rel = [], [], 0.0
            for i in range(total):
                a, la = step(native, i)
                if args.native_only:
                    lb, b = la, float("nan")
                else:
                    b, lb = step(composed, i)
                if i >= args.warmup:
                    tn.append(a), tc.append(b)
                    rel = max(rel, abs(la - lb) / abs(lb))
            row = {"nb": nb, "m": m, "native_ms_median": float(np.median(tn)), "composed_ms_median": float(np.median(tc)),
                   "native_over_composed": float(np.median(tn) / np.median(tc)), "max_rel_diff_of_the_two_losses": rel,
                   "native_ms_min": float(np.min(tn)), "composed_ms_min": float(np.min(tc)), "steps": args.steps, "warmup": args.warmup}
            result["shapes"].append(row)
            del model
            torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
