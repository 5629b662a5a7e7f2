"""What the likelihood tests share: the goldens of tests/golden/make_lik_golden.py composed into [rows, dy] problems, the
likelihood object of a golden group, and a Gauss-Hermite rule of any order for the closed-form and truncation checks."""
import math

import numpy as np
import torch

from gptorch_amd import likelihoods
from tests._util import load_npz

U = 2.0 ** -53
TINY = 2.0 ** -1022                # the smallest normal fp64 number
# 256 * 2^-53 * S: at most 64 sequential accumulations over the nodes, a reduction tree of at most 17 levels, and a few ulp per
# elementary function (erfcx, log, log1p, exp, lgamma) and per rounding of f_h = mu + sqrt(2 v) x_h, each relative to a term of S
BOUND = 256.0 * U
GOLD = load_npz("lik_cases.npz")
GROUPS = [str(n) for n in GOLD["names"]]
HS = [int(h) for h in GOLD["HS"]]
VS = [float(v) for v in GOLD["VS"]]
E = GOLD["mu"].shape[1]


def make_likelihood(g, H=None):
    name, (p0, p1) = GROUPS[g], GOLD["params"][g]
    if name == "probit" or name == "logit":
        lik = likelihoods.Bernoulli(link=name)
    elif name == "poisson":
        lik = likelihoods.Poisson()
    else:
        lik = likelihoods.StudentT(df=float(p0), scale=math.sqrt(float(p1)))
    if H is not None:
        lik.num_gauss_hermite_points = H
    return lik


def compose(g, ih, rows, dy):
    """rows x dy entries of group g at HS[ih]: row r has the variance VS[r % 4], its columns walk the entries.  -> dict of the
    inputs (mu, y [rows, dy], v [rows]) and what the rule gives: val, dmu [rows, dy], dv [rows] (summed over the row's columns),
    dp, each with the sum of the absolute values of its terms beside it (*_S)."""
    nv = len(VS)
    iv = np.arange(rows) % nv
    e = (np.arange(rows)[:, None] // nv + 3 * np.arange(dy)[None, :]) % E      # (40 rows: every (v, entry) pair in column 0)
    pick = lambda k: GOLD[k][g, ih][iv[:, None], e]
    out = dict(mu=GOLD["mu"][g][e], y=GOLD["y"][g][e], v=np.asarray(VS)[iv])
    out["val"], out["val_S"] = math.fsum(pick("val").ravel()), math.fsum(pick("val_S").ravel())
    out["dmu"], out["dmu_S"] = pick("dmu"), pick("dmu_S")
    out["dv"], out["dv_S"] = pick("dv").sum(1), pick("dv_S").sum(1)
    out["dp"], out["dp_S"] = math.fsum(pick("dp").ravel()), math.fsum(pick("dp_S").ravel())
    return out


def worst(got, want, S):
    """max |got - want| / (2^-53 S) over the entries; where S = 0 the number must be exact, and where 2^-53 S is below the
    normal range of fp64 (sigma(-750) = 1e-326: such numbers carry no relative precision) it must be below that range too."""
    got, want, S = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (got, want, S))
    err = np.abs(got - want)
    assert np.all(err[S == 0.0] == 0.0)
    tiny = S * U < TINY
    assert np.all(err[tiny] < TINY)
    if tiny.all():
        return 0.0
    return float(np.max(err[~tiny] / (U * S[~tiny])))


def rule(fn, mu, v, H):
    """pi^-1/2 sum_h w_h fn(mu + sqrt(2 v) x_h) with the H-node rule (any H), fp64 torch on the host."""
    x, w = np.polynomial.hermite.hermgauss(H)
    x, w = torch.tensor(x), torch.tensor(w / math.sqrt(math.pi))
    return (fn(mu.unsqueeze(-1) + torch.sqrt(2.0 * v).unsqueeze(-1) * x) * w).sum(-1)
