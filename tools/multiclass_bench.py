#!/usr/bin/env python3
"""GPU-box tool: loss(); backward() of a ten-class SVGP (likelihoods.MultiClass) on one MI355X with the data term from the fused
robust-max kernel (models/sparse_gpr.py NATIVE_EXPECTATION, csrc/multiclass.hip) against THE SAME bound with the data term from
the likelihood's torch route ([nb, H, C] intermediates and their autograd twins).  N = 1e6, d = 8, C = 10, Matern52, labels =
the largest of ten noisy linear scores; the two routes are interleaved step by step in one process on the same pre-drawn
minibatches; median [min, max] of each over the measured steps; one JSON line.  Beside the steps: the duration of one
gpn_lik_expect_robustmax call (both launches) at each batch size, by device events around a burst of calls.

    python tools/multiclass_bench.py [--shapes 1024x256,4096x1024,16384x2048] [--steps 15] [--warmup 5] [--out profiles/multiclass_step.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from gptorch_amd import _ops, kernels, likelihoods, rng  # noqa: E402
from gptorch_amd.models import SVGP, sparse_gpr  # noqa: E402


def stats(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts))}


def kernel_call_ms(nb, C, H, burst=50, repeats=7):
    """one gpn_lik_expect_robustmax call (every output) at nb rows: device events around `burst` back-to-back calls."""
    g = torch.Generator(device="cuda").manual_seed(5)
    f_mean = torch.randn(nb, C, dtype=torch.float64, device="cuda", generator=g)
    f_var = torch.rand(nb, dtype=torch.float64, device="cuda", generator=g) + 0.05
    labels = torch.randint(0, C, (nb,), device="cuda", generator=g).double()
    x, w = likelihoods.gauss_hermite(H, f_mean.device)
    out = []
    for _ in range(repeats + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(burst):
            _ops.lik_expect_robustmax(f_mean, f_var, labels, 1e-3, x, w)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / burst)
    return out[2:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--shapes", default="1024x256,4096x1024,16384x2048")
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multiclass_bench.py measures on the GPU; there is none here")
    if args.steps < 7:
        raise SystemExit("at least 7 measured steps")
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    n, d, C = args.n, args.d, args.classes
    x = rng.normal(0, (n, d))
    y = np.argmax(x @ rng.normal(1, (d, C)) + 0.3 * rng.normal(2, (n, C)), 1).astype(np.float64)[:, None]
    result = {"workload": "SVGP MultiClass(C=%d) Matern52 N=%d d=%d H=20 fp64, loss(); backward(), one MI355X, routes interleaved" % (C, n, d),
              "shapes": []}
    for nb, m in shapes:
        z = rng.normal(99, (m, d))
        np.random.seed(0)
        model = SVGP(x[:4000], y[:4000], kernels.Matern52(d, variance=1.0, length_scales=float(np.sqrt(d))), inducing_points=z,
                     likelihood=likelihoods.MultiClass(C), batch_size=nb)
        model.cuda()
        model.X, model.Y = torch.tensor(x).cuda(), torch.tensor(y).cuda()
        rs = np.random.RandomState(1)
        total = args.steps + args.warmup
        batches = [torch.as_tensor(rs.permutation(n)[:nb]).cuda() for _ in range(total)]

        def step(native, i):
            sparse_gpr.NATIVE_EXPECTATION = native
            xb, yb = model.X[batches[i]], model.Y[batches[i]]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.zero_grad()
            loss = model.loss(x=xb, y=yb)
            loss.backward()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, loss.item()
        tn, tt, rel = [], [], 0.0
        for i in range(total):
            order = (True, False) if i % 2 == 0 else (False, True)           # alternate which route goes first
            got = {nat: step(nat, i) for nat in order}
            if i >= args.warmup:
                tn.append(got[True][0]), tt.append(got[False][0])
                rel = max(rel, abs(got[True][1] - got[False][1]) / abs(got[False][1]))
        sparse_gpr.NATIVE_EXPECTATION = True
        sn, st = stats(tn), stats(tt)
        H = model.likelihood.num_gauss_hermite_points
        call = kernel_call_ms(nb, C, H)
        row = {"nb": nb, "m": m, "steps": args.steps, "warmup": args.warmup, "native": sn, "torch": st,
               "native_over_torch": sn["ms_median"] / st["ms_median"], "max_rel_diff_of_the_two_losses": rel,
               "robustmax_call_us_median": float(np.median(call)) * 1e3, "robustmax_call_us_min": float(np.min(call)) * 1e3,
               "special_function_evaluations_per_call": 2 * nb * (C - 1) * H,
               "native_range_not_above_torch_range": bool(sn["ms_min"] <= st["ms_max"])}
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del model
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
