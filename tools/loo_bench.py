#!/usr/bin/env python3
"""GPU-box tool: what the leave-one-out objective of GPR costs on one MI355X, beside the log marginal likelihood of the SAME
model in the same process.

Matern52, d = 8, dy = 1, N in {2048, 8192, 32768}.  Per N, interleaved round by round (host clock around work that ends in a device
synchronise; medians, minima, maxima and the inter-quartile range):

    loo_log_predictive    loo_log_predictive() under no_grad: factorisation, U = L^-T, P = U U^T, a, the per-point terms, w
    loo_loss_backward     loss(); backward() with objective="loo": the above + S = P diag(sqrt d), Q = S S^T, the gradient sweep
    lml_log_likelihood    log_likelihood() under no_grad (one assembly + one factorisation)
    lml_loss_backward     loss(); backward() with objective="lml" on the same data and hyper-parameters: the yardstick

and ratio_loss_backward = loo_loss_backward / lml_loss_backward (medians; the flop model says 2), plus the duration of each
native call of the leave-one-out forward and backward, by device events around a burst of calls.

    python tools/loo_bench.py [--sizes 2048,8192,32768] [--rounds 15] [--warmup 3] [--out profiles/loo_step.json]
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
from gptorch_amd.models import GPR  # noqa: E402


def stats(ts):
    q1, med, q3 = np.percentile(ts, [25, 50, 75])
    return {"ms_median": float(med), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "ms_iqr": float(q3 - q1)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def burst_ms(fn, burst, repeats=3):
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
    """each native call of the leave-one-out forward and backward at the model's hyper-parameters, in ms (device events, bursts)."""
    k = m.kernel
    n = m.X.shape[0]
    burst = 10 if n <= 4096 else (3 if n <= 8192 else 1)
    with torch.no_grad():
        var, ls, noise = k.variance.transform(), k.length_scales.transform(), m.likelihood.variance.transform()
        f = _ops.kernel_factor(k._kind, m.X, var, ls, noise, R=m.Y)
    kpad = _ops.round_up(n, 16)
    out = {"assembly_and_potrf": burst_ms(lambda: _ops.kernel_factor_async(k._kind, m.X, var, ls, noise, R=m.Y, factor=f), burst),
           "trtri_upper": burst_ms(lambda: _backward._upper_inverse(f), burst)}
    U = _backward._upper_inverse(f)
    out["kinv_UUt"] = burst_ms(lambda: _backward._kinv_lower(f, U), burst)
    Kinv = _backward._kinv_lower(f, U)
    at = _ops.gemm_nt(f.A[n:], U, 1, n, kpad, tri=_ops.TRI_B_UPPER)
    out["loo_terms"] = burst_ms(lambda: _ops.loo_terms(Kinv, at, n, 1), burst)
    Bt = _ops.padded_like_factor(f, 1)
    _, _, rootd, _ = _ops.loo_terms(Kinv, at, n, 1, qt=Bt)

    def w_pair():
        f.solve_right_lt(Bt, 1)
        return _ops.gemm_nt(Bt, U, 1, n, kpad, tri=_ops.TRI_B_UPPER)
    out["w_trsm_and_gemm"] = burst_ms(w_pair, burst)
    wt = w_pair()
    del U
    S = _ops.zeros(f.rows, f.ld, f.device)
    out["loo_scale"] = burst_ms(lambda: _ops.loo_scale(Kinv, rootd, n, S), burst)
    Q = torch.empty(_ops.round_up(n, 64), f.ld, dtype=torch.float64, device=f.device)
    out["syrk_SSt"] = burst_ms(lambda: _ops.gemm_nt(S, S, n, n, kpad, C=Q, lower=True), burst)
    out["loo_grad"] = burst_ms(lambda: _ops.loo_grad(k._kind, m.X, var, ls, Q, at, wt), burst)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,8192,32768")
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-native-calls", action="store_true", help="skip the per-call bursts (they hold three more N x N buffers)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loo_bench.py measures on the GPU; there is none here")
    d = args.d
    result = {"workload": "GPR Matern52 d=%d dy=1 fp64, objective=\"loo\" beside objective=\"lml\" on the same points and hyper-parameters, one "
                          "MI355X, legs interleaved round by round" % d, "sizes": []}

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(result, fh, indent=1)

    for n in (int(v) for v in args.sizes.split(",")):
        x, y = rng.make_regression(n, d, 1, seed=0)

        def model(objective):
            m = GPR(x, y, kernels.Matern52(d, variance=1.0, length_scales=float(np.sqrt(d))), likelihood=likelihoods.Gaussian(variance=0.05),
                    objective=objective)
            m.cuda()
            return m
        loo, lml = model("loo"), model("lml")

        def loo_value():
            with torch.no_grad():
                return loo.loo_log_predictive()

        def lml_value():
            with torch.no_grad():
                return lml.log_likelihood()

        def loss_backward(m):
            def run():
                m.zero_grad()
                loss = m.loss()
                loss.backward()
                return loss
            return run

        legs = {"loo_log_predictive": loo_value, "loo_loss_backward": loss_backward(loo), "lml_log_likelihood": lml_value,
                "lml_loss_backward": loss_backward(lml)}
        ts = {k: [] for k in legs}
        for r in range(args.rounds + args.warmup):
            for name, fn in legs.items():
                t, _ = timed(fn)
                if r >= args.warmup:
                    ts[name].append(t)
        row = {"n": n, "d": d, "rounds": args.rounds, "warmup": args.warmup}
        row.update({k: stats(v) for k, v in ts.items()})
        row["ratio_loss_backward"] = row["loo_loss_backward"]["ms_median"] / row["lml_loss_backward"]["ms_median"]
        row["ratio_value"] = row["loo_log_predictive"]["ms_median"] / row["lml_log_likelihood"]["ms_median"]
        del lml
        loo._holder.clear()
        torch.cuda.empty_cache()
        if not args.no_native_calls:
            row["native_call_ms"] = native_calls(loo)
        result["sizes"].append(row)
        print(json.dumps(row), flush=True)
        write()
        del loo
        torch.cuda.empty_cache()
    write()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
