#!/usr/bin/env python3
"""GPU-box tool: `loss(); backward()` of B EPGP restarts of one data set in lock step (batched_loss_and_grad ->
models/_ep_lockstep.py) against the same restarts evaluated one after the other (each model's own loss(); backward(): the code
path of the commit before the lock-step one).  Bernoulli-probit labels, Matern52, d = 8: tools/laplace_lockstep_bench.py's protocol.
Both COLD (every search starts at zero sites) and WARM (every search starts at the previous evaluation's sites: an optimiser's
steady state).
Usage: ep_lockstep_bench.py [n=<N>,B=<B> ...] [--reps R] [--out FILE] [--append]
The two forms alternate R times after a warm-up of each; the result is the median with the smallest and largest repeat.  Times
are host clocks around work that ends in a device synchronise.  --append: add the rows to those FILE already holds (one shape per
process, each under a time limit of its own).  Needs a GPU (there is no fallback)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from gptorch_amd import kernels, likelihoods, rng  # noqa: E402
from gptorch_amd.models import EPGP, batched_loss_and_grad  # noqa: E402
from gptorch_amd.models import _ep_lockstep as el  # noqa: E402
from gptorch_amd.models import _lockstep  # noqa: E402

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
out_path = option("--out", os.path.join(ROOT, "profiles", "ep_lockstep.json"))
cases = argv or ["n=512,B=64", "n=2048,B=16", "n=8192,B=8"]
if not torch.cuda.is_available():
    sys.exit("ep_lockstep_bench.py measures on a GPU; none found")


def models(n, B):
    x = rng.normal(11, (n, D))
    g = np.sin(1.3 * x[:, 0]) + 0.7 * np.cos(x[:, 1:].sum(1)) + 0.3 * x[:, 0]
    y = (rng.uniform(12, n) < 0.5 * (1.0 + np.tanh(1.2 * g))).astype(np.float64).reshape(n, 1)
    ms = []
    for b in range(B):
        # restarts: the variance over a decade, the length scale around sqrt(D)
        k = kernels.Matern52(D, variance=0.5 * 10.0 ** (b / max(B - 1, 1)), length_scales=float(np.sqrt(D)) * (0.6 + 0.8 * ((7 * b) % B) / B))
        m = EPGP(x, y, k, likelihoods.Bernoulli("probit"))
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


results = []
for case in cases:
    kv = dict(t.split("=") for t in case.split(","))
    n, B = int(kv["n"]), int(kv["B"])
    ms = models(n, B)
    grouped = sum(len(g) for _, g in _lockstep._ep_groups(ms))
    if grouped != B:
        sys.exit("n = %d: only %d of %d models are grouped (_ep_lockstep.supported): nothing to compare" % (n, grouped, B))

    def seq(cold):
        for m in ms:
            if cold:
                m.reset_sites()
            m.zero_grad()
            m.loss().backward()

    def lock(cold):
        for m in ms:
            if cold:
                m.reset_sites()
            m.zero_grad()
        batched_loss_and_grad(ms)

    row = {"n": n, "B": B, "d": D, "kernel": "Matern52", "likelihood": "Bernoulli(probit)", "reps": reps, "models_in_lock_step": grouped}
    for cold in (True, False):
        seq(True), lock(True)                    # warm-up of both forms (code objects, allocator, the lock-step buffers)
        if not cold:
            seq(False)                           # every model holds the sites of its parameters: the steady state
        t_seq, t_lock = [], []
        for _ in range(reps):                    # alternating: what else runs on the host hits both alike
            t_seq.append(timed(lambda: seq(cold)))
            sweeps = [m.ep_stats["sweeps"] for m in ms]
            before = dict(el.STATS)
            t_lock.append(timed(lambda: lock(cold)))
            stats = {k: el.STATS[k] - before[k] for k in before}
            assert not cold or sweeps == [m.ep_stats["sweeps"] for m in ms]         # the same searches, model by model
        s, l = summary(t_seq), summary(t_lock)
        tag = "cold" if cold else "warm"
        row[tag] = {"one_after_the_other": s, "lock_step": l, "ratio_of_medians": s["median_ms"] / l["median_ms"],
                    "sweeps": [min(sweeps), max(sweeps)], "lock_step_counters": stats}
        print("N %5d B %3d %s: one after the other %9.2f ms [%.2f, %.2f] | lock step %9.2f ms [%.2f, %.2f] -> %5.2fx   (sweeps %d-%d, %s)"
              % (n, B, tag, s["median_ms"], s["min_ms"], s["max_ms"], l["median_ms"], l["min_ms"], l["max_ms"], row[tag]["ratio_of_medians"],
                 min(sweeps), max(sweeps), stats), flush=True)
    results.append(row)
    del ms
    _lockstep.release_batch_buffers()
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
if append and os.path.exists(out_path):
    with open(out_path) as fh:
        results = json.load(fh)["results"] + results
with open(out_path, "w") as fh:
    json.dump({"tool": "tools/ep_lockstep_bench.py", "device": torch.cuda.get_device_name(0), "results": results}, fh, indent=1)
    fh.write("\n")
print("wrote %s" % out_path)
