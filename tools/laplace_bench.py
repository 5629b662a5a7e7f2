#!/usr/bin/env python3
"""GPU-box tool: what a LaplaceGP evaluation costs on one MI355X, beside GPR on the same points in the same process.

Bernoulli-probit, Matern52, d = 8, labels sign(sin(sum x)), N in {2048, 8192}.  Per N, interleaved round by round (host clock
around work that ends in a device synchronise; medians, minima and the inter-quartile range):

    laplace_cold          log_likelihood() from a = 0: `steps` Newton steps + the factorisation at the mode
    laplace_warm          log_likelihood() from the previous mode: 1 step + the factorisation at the mode
    newton_step_ms        (cold - warm) / (steps_cold - steps_warm): a DERIVED figure, one Newton step with its host read
    laplace_loss_backward loss(); backward() from the previous mode (what an optimiser iteration costs)
    gpr_log_likelihood    GPR.log_likelihood() of that N (one assembly + one factorisation)
    gpr_loss_backward     GPR loss(); backward()

and the duration of each native call of a step and of the backward, by device events around a burst of calls.

    python tools/laplace_bench.py [--sizes 2048,8192] [--rounds 15] [--warmup 3] [--out profiles/laplace_step.json]
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
from gptorch_amd import _backward, _ops, kernels, likelihoods, rng  # noqa: E402
from gptorch_amd.models import GPR, LaplaceGP, laplace  # noqa: E402


def stats(ts):
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return {"ms_median": float(med), "ms_min": float(np.min(ts)), "ms_iqr": float(q3 - q1)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def burst_ms(fn, burst, repeats=5):
    out = []
    for _ in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(burst):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / burst)
    return float(np.median(out[1:]))


def native_calls(m):
    """each native call of a Newton step and of the backward at the model's mode, in ms (device events, bursts)."""
    k = m.kernel
    with torch.no_grad():
        var, ls = k.variance.transform(), k.length_scales.transform()
        mode = laplace.find_mode(k._kind, m._lik_kind, m.X, m.Y.reshape(-1), m.mean_function(m.X).reshape(-1), var, ls)
    f, n = mode.factor, m.X.shape[0]
    burst = 20 if n <= 4096 else 5
    args = (k._kind, m.X, var, ls)
    out = {"lik_derivs": burst_ms(lambda: _ops.lik_derivs(m._lik_kind, mode.f, m.Y.reshape(-1)), burst),
           "laplace_matvec": burst_ms(lambda: _ops.laplace_matvec(*args, mode.a), burst),
           "laplace_system": burst_ms(lambda: _ops.laplace_system(*args, mode.s, f.A, f.ld), burst)}

    def refactor():
        _ops.laplace_system(*args, mode.s, f.A, f.ld)
        f.pack_rhs(mode.a.reshape(-1, 1))
        f.potrf(check=False)
    t_sys_potrf = burst_ms(refactor, burst)
    out["potrf_with_extra_row"] = t_sys_potrf - out["laplace_system"]
    out["backsub"] = burst_ms(lambda: _ops.backsub(f), burst)
    t_inv = burst_ms(lambda: _backward._kinv_lower(f, _backward._upper_inverse(f)), max(2, burst // 2))
    out["inverse_U_and_UUt"] = t_inv
    Binv = _backward._kinv_lower(f, _backward._upper_inverse(f))
    out["laplace_diag"] = burst_ms(lambda: _ops.laplace_diag(*args, mode.s, Binv), burst)
    out["laplace_grad"] = burst_ms(lambda: _ops.laplace_grad(*args, mode.s, Binv, mode.a, mode.d1, mode.d1), burst)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,8192")
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("laplace_bench.py measures on the GPU; there is none here")
    d = args.d
    result = {"workload": "LaplaceGP Bernoulli-probit Matern52 d=%d fp64 beside GPR (Gaussian) on the same points, one MI355X, "
                          "legs interleaved round by round" % d, "sizes": []}
    for n in (int(v) for v in args.sizes.split(",")):
        x, f = rng.make_regression(n, d, 1, seed=0)
        labels = (f > 0.0).astype(np.float64)
        lm = LaplaceGP(x, labels, kernels.Matern52(d, variance=1.0, length_scales=float(np.sqrt(d))), likelihoods.Bernoulli("probit"))
        gm = GPR(x, f, kernels.Matern52(d, variance=1.0, length_scales=float(np.sqrt(d))), likelihood=likelihoods.Gaussian(variance=0.05))
        lm.cuda()
        gm.cuda()

        def cold():
            lm.reset_mode()
            with torch.no_grad():
                return lm.log_likelihood()

        def warm():
            with torch.no_grad():
                return lm.log_likelihood()

        def lap_lb():
            lm.zero_grad()
            loss = lm.loss()
            loss.backward()
            return loss

        def gpr_ll():
            with torch.no_grad():
                return gm.log_likelihood()

        def gpr_lb():
            gm.zero_grad()
            loss = gm.loss()
            loss.backward()
            return loss

        legs = {"laplace_cold": cold, "laplace_warm": warm, "laplace_loss_backward": lap_lb, "gpr_log_likelihood": gpr_ll,
                "gpr_loss_backward": gpr_lb}
        ts = {k: [] for k in legs}
        steps = {}
        for r in range(args.rounds + args.warmup):
            for name, fn in legs.items():                 # (cold first: the warm legs start from its mode)
                t, _ = timed(fn)
                if name in ("laplace_cold", "laplace_warm"):
                    steps[name] = lm.newton_stats["steps"]
                if r >= args.warmup:
                    ts[name].append(t)
        row = {"n": n, "d": d, "rounds": args.rounds, "warmup": args.warmup, "steps_cold": steps["laplace_cold"],
               "steps_warm": steps["laplace_warm"]}
        row.update({k: stats(v) for k, v in ts.items()})
        per_step = (np.asarray(ts["laplace_cold"]) - np.asarray(ts["laplace_warm"])) / max(1, steps["laplace_cold"] - steps["laplace_warm"])
        row["newton_step_ms"] = dict(stats(per_step), derived="(cold - warm) / (steps_cold - steps_warm), round by round")
        row["native_call_ms"] = native_calls(lm)
        result["sizes"].append(row)
        print(json.dumps(row), flush=True)
        del lm, gm
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
