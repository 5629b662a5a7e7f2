#!/usr/bin/env python3
"""GPU-box tool: FITC (models/_fitc.py, csrc/fitc.hip) next to VFE on one MI355X -- log_likelihood() and loss(); backward() of
both models on the same data, inducing points and hyper-parameters, in one process, interleaved step by step; medians.  VFE is
the yardstick: FITC's forward is VFE's plus one HBM pass over every chunk, its backward adds one N x M x M contraction
(alpha [B^-1 | beta]), the chunk's right-solve (VFE's backward needs none) and one weighted accumulation.  The two row kernels
are also timed by themselves on one chunk (HIP events around repeated launches) for their achieved HBM bandwidth over their
algorithmic bytes (forward rows: 2 rows M 8 -- the chunk read and written back; backward rows: 5 rows M 8 -- alpha and T read,
T, alpha^T and (g alpha)^T written).

    python tools/fitc_bench.py [--shapes 1048576x1024,1000000x4096] [--d 8] [--steps 5] [--warmup 2] [--out profiles/fitc_step.json]
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
from gptorch_amd import _native, _ops, kernels, likelihoods, rng  # noqa: E402
from gptorch_amd.models import FITC, VFE  # noqa: E402

HBM_PEAK = 8.0e12      # bytes/s, MI355X data sheet


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def row_kernels(m, rows=65536, dy=1, reps=10):
    """ms per launch and achieved bytes/s of the two row kernels on one [rows, m] chunk of well-scaled random data."""
    dev = torch.device("cuda")
    lib = _native.lib()
    ptr, stream = _ops._ptr, _ops._stream(dev)
    mp, pp = _ops.round_up(m, 16), _ops.round_up(dy, 16)
    g = torch.Generator(device="cuda").manual_seed(1)
    src = torch.randn(rows, mp, dtype=torch.float64, device=dev, generator=g) / np.sqrt(2.0 * m)      # |a_i|^2 ~ 1/2 < kdiag = 1
    At = torch.empty_like(src)
    err = torch.randn(rows, dy, dtype=torch.float64, device=dev, generator=g)
    kd = torch.ones(1, dtype=torch.float64, device=dev)
    errT = torch.zeros(pp, rows, dtype=torch.float64, device=dev)
    lam = torch.empty(rows, dtype=torch.float64, device=dev)
    work = torch.empty(max(1, int(lib.gpn_fitc_forward_work_bytes(rows)) // 8), dtype=torch.float64, device=dev)
    out2 = torch.empty(2, dtype=torch.float64, device=dev)
    ldt = mp + pp
    T0 = torch.randn(rows, ldt, dtype=torch.float64, device=dev, generator=g) / m
    T = torch.empty_like(T0)
    beta = torch.randn(m, dy, dtype=torch.float64, device=dev, generator=g)
    r_out, g_out = torch.empty(rows, dy, dtype=torch.float64, device=dev), torch.empty(rows, dtype=torch.float64, device=dev)
    aT, gaT = torch.empty(mp, rows, dtype=torch.float64, device=dev), torch.empty(mp, rows, dtype=torch.float64, device=dev)

    def forward():
        _native.check(lib.gpn_fitc_forward_rows(stream, ptr(At), mp, rows, m, ptr(err), dy, ptr(kd), 0, 0.1, ptr(errT), rows, ptr(lam), ptr(work),
                                                ptr(out2)), "gpn_fitc_forward_rows")

    def backward():
        _native.check(lib.gpn_fitc_backward_rows(stream, ptr(src), mp, ptr(T), ldt, rows, m, ptr(beta), dy, dy, ptr(err), ptr(lam), ptr(r_out),
                                                 ptr(g_out), ptr(aT), ptr(gaT), rows), "gpn_fitc_backward_rows")
    out = {}
    for name, fn, restore, nbytes in (("fitc_forward_rows", forward, lambda: At.copy_(src), 2.0 * rows * m * 8),
                                      ("fitc_backward_rows", backward, lambda: T.copy_(T0), 5.0 * rows * m * 8)):
        ms = []
        for _ in range(reps + 2):
            restore()                                                       # (the kernels work in place)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = float(np.median(ms[2:]))
        out[name] = {"rows": rows, "m": m, "ms_median": med, "algorithmic_bytes": nbytes, "bytes_per_s": nbytes / (med * 1e-3),
                     "frac_hbm_peak": nbytes / (med * 1e-3) / HBM_PEAK}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1048576x1024,1000000x4096")
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-row-kernels", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    d = args.d
    result = {"workload": "FITC and VFE, Matern52 d=%d dy=1 fp64, one MI355X, same process, interleaved" % d, "shapes": []}
    for n, m in [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]:
        x, y = rng.make_regression(n, d, 1, seed=0)
        z = rng.normal(99, (m, d))
        models = {}
        for name, cls in (("fitc", FITC), ("vfe", VFE)):
            mod = cls(x[:4000], y[:4000], kernels.Matern52(d, variance=1.0, length_scales=float(np.sqrt(d))), inducing_points=z.copy(),
                      likelihood=likelihoods.Gaussian(variance=0.1))
            mod.cuda()
            models[name] = mod
        X, Y = torch.tensor(x).cuda(), torch.tensor(y).cuda()
        for mod in models.values():
            mod.X, mod.Y = X, Y

        def forward(mod):
            with torch.no_grad():
                return mod.log_likelihood().item()

        def step(mod):
            mod.zero_grad()
            loss = mod.loss()
            loss.backward()
            return loss.item()
        t = {k: [] for k in ("fitc_forward", "vfe_forward", "fitc_step", "vfe_step")}
        values = {}
        for i in range(args.steps + args.warmup):
            for name in ("fitc", "vfe"):
                a, values[name + "_log_likelihood"] = timed(lambda: forward(models[name]))
                b, _ = timed(lambda: step(models[name]))
                if i >= args.warmup:
                    t[name + "_forward"].append(a), t[name + "_step"].append(b)
        row = {"n": n, "m": m, "d": d, "steps": args.steps, "warmup": args.warmup}
        row.update({k + "_ms_median": float(np.median(v)) for k, v in t.items()})
        row.update({k + "_ms_min": float(np.min(v)) for k, v in t.items()})
        row["fitc_over_vfe_forward"] = row["fitc_forward_ms_median"] / row["vfe_forward_ms_median"]
        row["fitc_over_vfe_step"] = row["fitc_step_ms_median"] / row["vfe_step_ms_median"]
        row.update(values)
        del models, X, Y
        torch.cuda.empty_cache()
        if not args.no_row_kernels:
            row["row_kernels"] = row_kernels(m)
        result["shapes"].append(row)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
