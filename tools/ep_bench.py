#!/usr/bin/env python3
"""GPU-box tool: what an EPGP evaluation costs on one MI355X, beside LaplaceGP on the same points in the same process.

Bernoulli-probit, Matern52, d = 8, labels sign(f) of a smooth f, N in {2048, 8192}.  Per N, interleaved round by round (host clock
around work that ends in a device synchronise; medians, minima and maxima):

    ep_cold               log_likelihood() from tau = nu = 0: `sweeps` sweeps + the factorisation at the sites
    ep_warm               log_likelihood() from the previous sites: 1 sweep + the factorisation at the sites
    ep_sweep_ms           (cold - warm) / (sweeps_cold - sweeps_warm): a DERIVED figure, one sweep with its host read
    ep_loss_backward_cold loss(); backward() after reset_sites()
    ep_loss_backward_warm loss(); backward() from the previous sites (what an optimiser iteration costs)
    laplace_cold / laplace_warm / newton_step_ms    the same three for LaplaceGP (tools/laplace_bench.py's legs)
    laplace_loss_backward loss(); backward() from the previous mode

and the duration of each native call of a sweep, by device events around a burst of calls, with the share of a sweep that
gpn_ep_sites and the N^2 passes (the two matvecs, the assembly, the back-substitution, the diagonal) take.

    python tools/ep_bench.py [--sizes 2048,8192] [--rounds 15] [--warmup 3] [--out profiles/ep_step.json]
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
from gptorch_amd.models import EPGP, LaplaceGP, ep  # noqa: E402


def stats(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts))}


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
    """each native call of a sweep at the model's converged sites, in ms (device events, bursts)."""
    k = m.kernel
    with torch.no_grad():
        var, ls = k.variance.transform(), k.length_scales.transform()
        y, mean = m.Y.reshape(-1), m.mean_function(m.X).reshape(-1)
        st = ep.find_sites(k._kind, m._lik_kind, m.X, y, mean, var, ls)
    f, n = st.factor, m.X.shape[0]
    burst = 20 if n <= 4096 else 5
    args = (k._kind, m.X, var, ls)
    out = {"ep_sites": burst_ms(lambda: _ops.ep_sites(m._lik_kind, y, mean, st.mu, st.sigma2, st.tau, st.nu, m.damping, want_moments=False), burst),
           "laplace_matvec": burst_ms(lambda: _ops.laplace_matvec(*args, st.a), burst),
           "laplace_system": burst_ms(lambda: _ops.laplace_system(*args, st.s, f.A, f.ld), burst)}

    def refactor():
        _ops.laplace_system(*args, st.s, f.A, f.ld)
        f.pack_rhs(st.a.reshape(-1, 1))
        f.potrf(check=False)
    out["potrf_with_extra_row"] = burst_ms(refactor, burst) - out["laplace_system"]
    out["backsub"] = burst_ms(lambda: _ops.backsub(f), burst)
    out["inverse_U_and_UUt"] = burst_ms(lambda: _backward._kinv_lower(f, _backward._upper_inverse(f)), max(2, burst // 2))
    Binv = _backward._kinv_lower(f, _backward._upper_inverse(f))
    out["laplace_diag"] = burst_ms(lambda: _ops.laplace_diag(*args, st.s, Binv), burst)
    small = out["ep_sites"] + 2.0 * out["laplace_matvec"] + out["laplace_system"] + out["backsub"] + out["laplace_diag"]
    total = small + out["potrf_with_extra_row"] + out["inverse_U_and_UUt"]
    out["sweep_sum"] = total
    out["ep_sites_and_n2_passes_share"] = small / total
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
        raise SystemExit("ep_bench.py measures on the GPU; there is none here")
    d = args.d
    result = {"workload": "EPGP beside LaplaceGP, Bernoulli-probit Matern52 d=%d fp64 on the same points, one MI355X, legs interleaved "
                          "round by round" % d, "sizes": []}
    for n in (int(v) for v in args.sizes.split(",")):
        x, f = rng.make_regression(n, d, 1, seed=0)
        labels = (f > 0.0).astype(np.float64)

        def kern():
            return kernels.Matern52(d, variance=1.0, length_scales=float(np.sqrt(d)))

        em = EPGP(x, labels, kern(), likelihoods.Bernoulli("probit"))
        lm = LaplaceGP(x, labels, kern(), likelihoods.Bernoulli("probit"))
        em.cuda()
        lm.cuda()

        def value(m, reset):
            def run():
                if reset:
                    reset(m)
                with torch.no_grad():
                    return m.log_likelihood()
            return run

        def loss_backward(m, reset):
            def run():
                if reset:
                    reset(m)
                m.zero_grad()
                loss = m.loss()
                loss.backward()
                return loss
            return run

        legs = {"ep_cold": value(em, EPGP.reset_sites), "ep_warm": value(em, None),
                "laplace_cold": value(lm, LaplaceGP.reset_mode), "laplace_warm": value(lm, None),
                "ep_loss_backward_cold": loss_backward(em, EPGP.reset_sites), "ep_loss_backward_warm": loss_backward(em, None),
                "laplace_loss_backward": loss_backward(lm, None)}
        ts = {k: [] for k in legs}
        count = {}
        for r in range(args.rounds + args.warmup):
            for name, fn in legs.items():                 # (a cold leg first: the warm leg after it starts from its state)
                t, _ = timed(fn)
                if name.startswith("ep_"):
                    count[name] = em.ep_stats["sweeps"]
                elif name in ("laplace_cold", "laplace_warm"):
                    count[name] = lm.newton_stats["steps"]
                if r >= args.warmup:
                    ts[name].append(t)
        row = {"n": n, "d": d, "rounds": args.rounds, "warmup": args.warmup, "sweeps_cold": count["ep_cold"], "sweeps_warm": count["ep_warm"],
               "sweeps_loss_backward_cold": count["ep_loss_backward_cold"], "sweeps_loss_backward_warm": count["ep_loss_backward_warm"],
               "newton_steps_cold": count["laplace_cold"], "newton_steps_warm": count["laplace_warm"], "ep_stalled": bool(em.ep_stats["stalled"])}
        row.update({k: stats(v) for k, v in ts.items()})
        sweep = (np.asarray(ts["ep_cold"]) - np.asarray(ts["ep_warm"])) / max(1, count["ep_cold"] - count["ep_warm"])
        step = (np.asarray(ts["laplace_cold"]) - np.asarray(ts["laplace_warm"])) / max(1, count["laplace_cold"] - count["laplace_warm"])
        row["ep_sweep_ms"] = dict(stats(sweep), derived="(cold - warm) / (sweeps_cold - sweeps_warm), round by round")
        row["newton_step_ms"] = dict(stats(step), derived="(cold - warm) / (steps_cold - steps_warm), round by round")
        row["sweep_over_newton_step"] = float(np.median(sweep) / np.median(step))
        row["native_call_ms"] = native_calls(em)
        result["sizes"].append(row)
        print(json.dumps(row), flush=True)
        del em, lm
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
