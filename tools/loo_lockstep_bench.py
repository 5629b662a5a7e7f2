#!/usr/bin/env python3
"""GPU-box tool: `loss(); backward()` of B leave-one-out restarts of one data set through batched_loss_and_grad against the same
restarts evaluated one after the other (each model's own loss(); backward()).  GPR(objective="loo"), Matern52, d = 8, dy = 1:
tools/ep_lockstep_bench.py's protocol.
The script uses the public API only, so it runs unchanged on the commit BEFORE the lock-step one, where batched_loss_and_grad walks
the LOO models one by one: that commit's `batched_loss_and_grad` column is the baseline of the comparison; the in-build
`one_after_the_other` column is recorded beside it as a cross-check.
Usage: loo_lockstep_bench.py [n=<N>,B=<B> ...] [--reps R] [--label TEXT] [--out FILE] [--append]
The two forms alternate R times after a warm-up of each; the result is the median with the smallest and largest repeat.  Times
are host clocks around work that ends in a device synchronise.  After the timing the two forms' losses and gradients are compared
bit for bit (`bit_identical`).  --label: which build the rows come from ("parent", "lock-step").  --append: add the rows to those FILE
already holds (one shape per process, each under a time limit of its own).  Needs a GPU (there is no fallback)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from gptorch_amd import kernels, likelihoods, rng  # noqa: E402
from gptorch_amd.models import GPR, batched_loss_and_grad, release_batch_buffers  # noqa: E402

D = 8
argv = sys.argv[1:]


def option(name, default):
    if name in argv:
        at = argv.index(name)
        value = argv[at + 1]
        del argv[at:at + 2]
        return value
    return default


append = "--append" in argv
if append:
    argv.remove("--append")
reps = int(option("--reps", 7))
label = option("--label", "")
out_path = option("--out", os.path.join(ROOT, "profiles", "loo_lockstep.json"))
cases = argv or ["n=512,B=64", "n=2048,B=16", "n=8192,B=8"]
if not torch.cuda.is_available():
    sys.exit("loo_lockstep_bench.py measures on a GPU; none found")


def models(n, B):
    x, y = rng.make_regression(n, D, 1, seed=11)
    ms = []
    for b in range(B):
        # restarts: the variance over a decade, the length scale around sqrt(D), the noise over a decade
        k = kernels.Matern52(D, variance=0.5 * 10.0 ** (b / max(B - 1, 1)), length_scales=float(np.sqrt(D)) * (0.6 + 0.8 * ((7 * b) % B) / B))
        m = GPR(x, y, k, likelihood=likelihoods.Gaussian(variance=0.02 * 10.0 ** (((3 * b) % B) / B)), objective="loo")
        m.cuda()
        ms.append(m)
    for m in ms[1:]:
        m.X, m.Y = ms[0].X, ms[0].Y
    return ms


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(ts):
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}


def grads(ms):
    return [None if p.grad is None else p.grad.detach().clone() for m in ms for p in m.parameters()]


results = []
for case in cases:
    kv = dict(t.split("=") for t in case.split(","))
    n, B = int(kv["n"]), int(kv["B"])
    ms = models(n, B)

    def seq():
        out = []
        for m in ms:
            m.zero_grad()
            loss = m.loss()
            loss.backward()
            out.append(loss.detach())
        return out

    def batched():
        for m in ms:
            m.zero_grad()
        return batched_loss_and_grad(ms)

    seq(), batched()                             # warm-up of both forms (code objects, allocator, the lock-step buffers)
    t_seq, t_bat = [], []
    for _ in range(reps):                        # alternating: what else runs on the host hits both alike
        t_seq.append(timed(seq))
        t_bat.append(timed(batched))
    want, g_want = seq(), grads(ms)
    got, g_got = batched(), grads(ms)
    same = all(torch.equal(a, b) for a, b in zip(got, want)) and \
        all((a is None) == (b is None) and (a is None or torch.equal(a, b)) for a, b in zip(g_got, g_want))
    s, l = summary(t_seq), summary(t_bat)
    row = {"label": label, "n": n, "B": B, "d": D, "dy": 1, "kernel": "Matern52", "objective": "loo", "reps": reps,
           "one_after_the_other": s, "batched_loss_and_grad": l, "ratio_of_medians": s["median_ms"] / l["median_ms"],
           "bit_identical": bool(same), "peak_memory_gb": torch.cuda.max_memory_allocated() / 2.0 ** 30}
    print("%s N %5d B %3d: one after the other %9.2f ms [%.2f, %.2f] | batched_loss_and_grad %9.2f ms [%.2f, %.2f] -> %5.2fx   bit-identical %s"
          % (label, n, B, s["median_ms"], s["min_ms"], s["max_ms"], l["median_ms"], l["min_ms"], l["max_ms"], row["ratio_of_medians"], same),
          flush=True)
    results.append(row)
    del ms
    release_batch_buffers()
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
if append and os.path.exists(out_path):
    with open(out_path) as fh:
        results = json.load(fh)["results"] + results
with open(out_path, "w") as fh:
    json.dump({"tool": "tools/loo_lockstep_bench.py", "device": torch.cuda.get_device_name(0), "results": results}, fh, indent=1)
    fh.write("\n")
print("wrote %s" % out_path)
