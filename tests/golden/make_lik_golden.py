"""Goldens of the Gauss-Hermite expectations of the non-Gaussian likelihoods (gptorch_amd/likelihoods.py, csrc/lik.hip), in
40-digit arithmetic (mpmath) -> tests/golden/lik_cases.npz.

    python tests/golden/make_lik_golden.py

What is stored is the SAME-RULE expectation: the sum over the very nodes x_h and weights w_h that numpy's hermgauss(H) returns
(taken as exact doubles), of the exactly evaluated log-density at f_h = mu + sqrt(2 v) x_h -- so a test measures the rounding
of an implementation of the rule, not the rule's truncation error.  Per entry (one (mu, y) pair under one variance v):

    val = pi^-1/2 sum_h w_h logp(f_h, y)      dmu = pi^-1/2 sum_h w_h logp'(f_h)
    dv  = pi^-1/2 sum_h w_h logp'(f_h) x_h / sqrt(2 v)      dp = pi^-1/2 sum_h w_h dlogp/dparam (Student-t: param = scale^2)

and beside each number the sum S of the absolute values of its terms (val_S, dmu_S, dv_S, dp_S): the scale its rounding
errors are measured in.  Poisson's expectation is its closed form y mu - exp(mu + v/2) - lgamma(y + 1) (the same for every H).

Layout: groups G (a likelihood kind with its parameters) x H in HS x v in VS x entries E; arrays [G, len(HS), len(VS), E].
An implementation under test composes rows from entries that share v (dy columns per row) and sums what it expects.
"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 40
HS = [1, 20, 64]
VS = [1.0e-6, 0.01, 1.0, 3.0]
PROBIT, LOGIT, POISSON, STUDENT_T = 0, 1, 2, 3
# (name, kind, (param0, param1), [(mu, y), ...]) -- ten entries per group
GROUPS = [
    # probit arguments z = (2y - 1) mu from -38 to +9: both branches, both tails
    ("probit", PROBIT, (0.0, 0.0), [(-38.0, 1.0), (-20.0, 1.0), (-5.0, 1.0), (-0.3, 1.0), (0.0, 0.0), (0.7, 0.0), (3.0, 1.0), (9.0, 1.0),
                                    (9.0, 0.0), (38.0, 0.0)]),
    # logit at +-750 (exp(750) overflows a double) and around the centre
    ("logit", LOGIT, (0.0, 0.0), [(-750.0, 1.0), (-750.0, 0.0), (750.0, 1.0), (750.0, 0.0), (-30.0, 1.0), (-2.0, 1.0), (0.0, 0.0), (0.5, 1.0),
                                  (30.0, 0.0), (36.5, 1.0)]),
    # Poisson: y = 0, small counts, large counts near and away from their rate
    ("poisson", POISSON, (0.0, 0.0), [(-3.0, 0.0), (0.5, 0.0), (5.0, 0.0), (1.0, 3.0), (-1.0, 2.0), (2.5, 17.0), (13.8, 1.0e6), (12.0, 1.0e6),
                                      (20.0, 1.0e9), (6.9, 1000.0)]),
    # Student-t (df, scale^2): targets 50 scales away on both sides, and near the mean
    ("student_t_default", STUDENT_T, (3.0, 1.0), [(0.0, 50.0), (0.0, -50.0), (0.2, 0.1), (-1.0, 2.0), (4.0, 4.0), (10.0, -40.0), (-0.5, -0.25),
                                                  (1.0e-3, 0.0), (7.0, 9.5), (-3.0, 1.0)]),
    ("student_t_narrow", STUDENT_T, (4.5, 0.09), [(0.0, 15.0), (0.0, -15.0), (0.2, 0.1), (-1.0, 2.0), (4.0, 4.0), (10.0, -5.0), (-0.5, -0.25),
                                                  (1.0e-3, 0.0), (7.0, 7.3), (-3.0, -2.9)]),
]


def log_ndtr(z):
    return mp.log(mp.erfc(-z / mp.sqrt(2)) / 2)


def terms(kind, par, f, y):
    """-> (logp, [its terms]), (dlogp/df, [terms]), (dlogp/dparam, [terms]) at one point, all mpf."""
    if kind == PROBIT:
        s = 2 * y - 1
        z = s * f
        lp = log_ndtr(z)
        d = s * mp.exp(-z * z / 2 - lp) / mp.sqrt(2 * mp.pi)
        return (lp, [lp]), (d, [d]), (mp.mpf(0), [])
    if kind == LOGIT:
        s = 2 * y - 1
        t = s * f
        lp = -mp.log1p(mp.exp(-t)) if t > -1000 else t - mp.log1p(mp.exp(t))
        d = s / (1 + mp.exp(t))
        return (lp, [lp]), (d, [d]), (mp.mpf(0), [])
    nu, s2 = mp.mpf(par[0]), mp.mpf(par[1])
    r = y - f
    parts = [mp.loggamma((nu + 1) / 2), -mp.loggamma(nu / 2), -mp.log(nu * mp.pi * s2) / 2, -(nu + 1) / 2 * mp.log1p(r * r / (nu * s2))]
    d = (nu + 1) * r / (nu * s2 + r * r)
    dparts = [-1 / (2 * s2), (nu + 1) / 2 * r * r / (s2 * (nu * s2 + r * r))]
    return (sum(parts), parts), (d, [d]), (sum(dparts), dparts)


def entry(kind, par, H, x, w, mu, v, y):
    mu, v, y = mp.mpf(mu), mp.mpf(v), mp.mpf(y)
    if kind == POISSON:
        m = mp.exp(mu + v / 2)
        parts = [y * mu, -m, -mp.loggamma(y + 1)]
        return dict(val=sum(parts), val_S=sum(abs(p) for p in parts), dmu=y - m, dmu_S=abs(y) + m, dv=-m / 2, dv_S=m / 2,
                    dp=mp.mpf(0), dp_S=mp.mpf(0))
    out = {k: mp.mpf(0) for k in ("val", "val_S", "dmu", "dmu_S", "dv", "dv_S", "dp", "dp_S")}
    sd = mp.sqrt(2 * v)
    c = 1 / mp.sqrt(mp.pi)
    for h in range(H):
        xh, wh = mp.mpf(float(x[h])), mp.mpf(float(w[h])) * c
        (lp, lpt), (d, _), (dp, dpt) = terms(kind, par, mu + sd * xh, y)
        out["val"] += wh * lp
        out["val_S"] += wh * sum(abs(t) for t in lpt)
        out["dmu"] += wh * d
        out["dmu_S"] += wh * abs(d)
        out["dv"] += wh * d * xh / sd
        out["dv_S"] += wh * abs(d * xh / sd)
        out["dp"] += wh * dp
        out["dp_S"] += wh * sum(abs(t) for t in dpt)
    return out


def main():
    G, E = len(GROUPS), len(GROUPS[0][3])
    keys = ("val", "val_S", "dmu", "dmu_S", "dv", "dv_S", "dp", "dp_S")
    arrays = {k: np.zeros((G, len(HS), len(VS), E)) for k in keys}
    rules = {H: np.polynomial.hermite.hermgauss(H) for H in HS}
    for g, (name, kind, par, pts) in enumerate(GROUPS):
        assert len(pts) == E
        for ih, H in enumerate(HS):
            x, w = rules[H]
            for iv, v in enumerate(VS):
                for e, (mu, y) in enumerate(pts):
                    r = entry(kind, par, H, x, w, mu, v, y)
                    for k in keys:
                        arrays[k][g, ih, iv, e] = float(r[k])
        print("group %-18s done" % name)
    out = dict(arrays)
    out["names"] = np.array([g[0] for g in GROUPS])
    out["kind"] = np.array([g[1] for g in GROUPS], dtype=np.int64)
    out["params"] = np.array([g[2] for g in GROUPS], dtype=np.float64)
    out["mu"] = np.array([[p[0] for p in g[3]] for g in GROUPS], dtype=np.float64)
    out["y"] = np.array([[p[1] for p in g[3]] for g in GROUPS], dtype=np.float64)
    out["HS"] = np.array(HS, dtype=np.int64)
    out["VS"] = np.array(VS, dtype=np.float64)
    for H in HS:
        out["nodes_%d" % H], out["weights_%d" % H] = rules[H]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lik_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
