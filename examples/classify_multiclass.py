#!/usr/bin/env python3
"""Multi-class classification with SVGP and the robust-max likelihood (needs an MI355X).

Three classes in the plane -- three blobs with some overlap -- fitted by a sparse variational GP with one latent function per
class (likelihoods.MultiClass); the data term and its gradients come from one fused kernel per step.  Prints the bound before and
after, the training accuracy and the class probabilities at the blobs' centres.
Usage: python examples/classify_multiclass.py [N=600] [iterations=150]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from gptorch_amd import kernels, likelihoods, rng  # noqa: E402
from gptorch_amd.models import SVGP  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 600
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 150
centres = np.array([[0.0, 2.0], [-2.0, -1.5], [2.0, -1.5]])
labels = np.arange(n) % 3
x = centres[labels] + 0.8 * rng.normal(0, (n, 2))
y = labels.astype(np.float64)[:, None]                       # ONE column of class indices 0, 1, 2

np.random.seed(0)
model = SVGP(x, y, kernels.Rbf(2), num_inducing_points=30, likelihood=likelihoods.MultiClass(3))
model.cuda()
losses, seconds = model.optimize(method="Adam", max_iter=iters, learning_rate=0.05, verbose=False)
p, _ = model.predict_y(x)                                    # [n, 3] class probabilities
accuracy = float(np.mean(np.argmax(p, 1) == labels))
print("bound %.2f -> %.2f in %d Adam steps (%.2f s)" % (-losses[0], -losses[-1], iters, seconds))
print("training accuracy %.3f" % accuracy)
print("class probabilities at the centres:\n%s" % np.round(model.predict_y(centres)[0], 3))
