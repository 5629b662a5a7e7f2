#!/usr/bin/env python3
"""Model selection by leave-one-out cross-validation, in closed form (needs an MI355X).

A misspecified model -- a smooth Rbf prior on data with a kink -- fitted twice on the same points: on the log marginal likelihood
(the reference's only objective) and on the leave-one-out log predictive density (Rasmussen & Williams 5.4.2), which needs no
fold: every held-out mean and variance comes from the one inverse of the fit.  Both models are then scored by both criteria and
by the held-out residuals of loo_predict().
Usage: python examples/loo_model_selection.py [N=2000] [iterations=60]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from gptorch_amd import kernels, rng  # noqa: E402
from gptorch_amd.models import GPR, multi_start_optimize  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 60
d = 2
x = rng.normal(0, (n, d))
y = (np.abs(x[:, :1]) + 0.3 * np.sin(3.0 * x[:, 1:2])) + 0.1 * rng.normal(1, (n, 1))     # |x|: a kink no Rbf sample path has

for objective in ("lml", "loo"):
    m = GPR(x, y, kernels.Rbf(d, ARD=True), objective=objective)
    m.cuda()
    m.optimize(method="Adam", max_iter=iters, learning_rate=0.05, verbose=False)
    mean, var = m.loo_predict()
    resid = (mean - m.Y).cpu().numpy()
    print("fitted on %s: LML %.2f  L_LOO %.2f  noise %.4f  held-out RMSE %.4f  mean held-out variance %.4f"
          % (objective, m.log_likelihood().item(), m.loo_log_predictive().item(), m.likelihood.variance.transform().item(),
             float(np.sqrt(np.mean(resid ** 2))), float(var.mean().item())))

# A misspecified model is where one tries several starting points: four leave-one-out restarts in ONE multi_start_optimize call.
# Equal-shape objective="loo" models share every launch of an iteration (one lock-step evaluation; each restart keeps its own
# optimiser and follows, bit for bit, the trajectory its own optimize() would).
restarts = [GPR(x, y, kernels.Rbf(d, variance=v, length_scales=np.full(d, ell), ARD=True), objective="loo") for v, ell in ((0.3, 0.5), (1.0, 1.0), (3.0, 2.0), (10.0, 0.3))]
for m in restarts:
    m.cuda()
losses, seconds = multi_start_optimize(restarts, method="Adam", max_iter=iters, learning_rate=0.05, verbose=False)
best = int(np.argmin(losses[:, -1]))
print("4 leave-one-out restarts in lock step: %.2f s; final -L_LOO %s; best restart %d, noise %.4f"
      % (seconds, np.round(losses[:, -1], 2).tolist(), best, restarts[best].likelihood.variance.transform().item()))
