#!/usr/bin/env python3
"""Model selection by k-fold cross-validation, in closed form (needs an MI355X).

A misspecified model -- a smooth Rbf prior on data with a kink -- fitted three times on the same points: on the log marginal
likelihood (the reference's only objective), on the leave-one-out log predictive density and on the k-fold log predictive
density, which scores every fold JOINTLY (the held-out points of a fold with their covariance) given all the other folds.  No
fold is refitted: every held-out block comes from the diagonal blocks of the one inverse of the fit.  Each model is then scored
by all three criteria and by the held-out residuals of kfold_predict().
The folds are a shuffled partition: an int k would mean contiguous blocks in data order.
Usage: python examples/kfold_model_selection.py [N=2000] [k=5] [iterations=60]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from gptorch_amd import kernels, rng  # noqa: E402
from gptorch_amd.models import GPR  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
k = int(sys.argv[2]) if len(sys.argv) > 2 else 5
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 60
d = 2
x = rng.normal(0, (n, d))
y = (np.abs(x[:, :1]) + 0.3 * np.sin(3.0 * x[:, 1:2])) + 0.1 * rng.normal(1, (n, 1))     # |x|: a kink no Rbf sample path has
folds = np.array_split(np.argsort(rng.uniform(2, n), kind="stable"), k)

for objective in ("lml", "loo", "kfold"):
    m = GPR(x, y, kernels.Rbf(d, ARD=True), objective=objective, **(dict(folds=folds) if objective == "kfold" else {}))
    m.cuda()
    m.optimize(method="Adam", max_iter=iters, learning_rate=0.05, verbose=False)
    mean, var = m.kfold_predict(folds=folds)
    resid = (mean - m.Y).cpu().numpy()
    print("fitted on %-5s: LML %.2f  L_LOO %.2f  L_%d-fold %.2f  noise %.4f  held-out RMSE %.4f  mean held-out variance %.4f"
          % (objective, m.log_likelihood().item(), m.loo_log_predictive().item(), k, m.kfold_log_predictive(folds=folds).item(),
             m.likelihood.variance.transform().item(), float(np.sqrt(np.mean(resid ** 2))), float(var.mean().item())))
