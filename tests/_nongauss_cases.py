"""
TEST INFRASTRUCTURE ONLY -- the LaplaceGP and EPGP model cases of tests/test_gpu_nongauss_kinds.py for the kinds no older golden
case holds (Matern32, Exp, Periodic): their inputs, and the dense host oracles' numbers.  Host only.

LaplaceGP: the oracle runs where it is asked for, in long double and in fp64 (under a second per case).  EPGP: the long-double
sweep takes several seconds, so tests/golden/make_nongauss_kinds_golden.py stores its numbers, the fp64 oracle's distance e64 and
its sweep count in tests/golden/nongauss_kinds_cases.npz; tests/test_kind_ref_host.py re-runs the fp64 oracle against the fixture.

gptorch_amd never imports this module.
"""
import json

import numpy as np

from gptorch_amd import rng
from tests import _laplace_oracle as lo
from tests import _refine_ref as rr
from tests import _xref as xr

GOLDEN_NAME = "nongauss_kinds_cases.npz"

# ---- the tile-kernel cases: shapes, inputs and the references of K, K v, diag and the gradient sweep ---------------------------------
KINDS = ("Rbf", "Matern52", "Matern32", "Exp", "Periodic")
SIZES = (1, 64, 65, 129)                     # one row, a full tile, a tile and a row, two tiles and a row
DIMS = {k: ((1, 2) if k == "Periodic" else (1, 17, 33)) for k in KINDS}      # 17, 33: a second and a third 16-coordinate stage
TILE_CASES = [(k, n, d, ard) for k in KINDS for n in SIZES for d in DIMS[k] for ard in (False, True)]
LD = xr.LD


def problem(kind, n, d, ard):
    """planted points and hyper-parameters; the length scales grow with sqrt(d) so that r stays O(1) between random rows."""
    seed = 100 * KINDS.index(kind) + 7 * n + d + int(ard)
    ls = np.atleast_1d(rr.length_scales(d, ard, seed, 0.9 * np.sqrt(d)))
    full_ls = ls if ard else np.full(d, ls[0])
    return rr.points(seed + 1, n, d, full_ls[0]), rr.VAR, ls, full_ls, seed


def spd(n, seed):
    g = rng.normal(seed, (n, n + 3))
    return g @ g.T / (n + 3) + 0.5 * np.eye(n)


def tile_inputs(kind, n, d, ard):
    """everything test_tile_kernels_of_every_kind feeds the entry points for its case (kind, n, d, ard)."""
    x, var, ls, full_ls, seed = problem(kind, n, d, ard)
    a, u, d1, vec = (rng.normal(seed + 3 + k, (n,)) for k in range(4))
    return {"x": x, "var": var, "ls": ls, "full_ls": full_ls, "ard": ard, "s": 0.05 + 2.0 * rng.uniform(seed + 2, n), "a": a, "u": u, "d1": d1,
            "vec": vec, "Binv": spd(n, seed + 9)}


def tile_refs(t, kind):
    """{output: (long-double value, tolerance, metric)} of K, K v, diag and the gradient sweep on the inputs t for a NAMED kind:
    xr.tol(e64, "K" | "dense_grad") with e64 from the fp64 statement of the same sums (kernel, B and products in fp64)."""
    x, var, ls, full_ls, ard = t["x"], t["var"], t["ls"], t["full_ls"], t["ard"]
    d = x.shape[1]

    def host(dt):
        Km, Bm = lo.kern(kind, x, None, var, full_ls.astype(dt), dt)
        sd, Bd = t["s"].astype(dt), t["Binv"].astype(dt)
        a, u, d1 = (t[k].astype(dt) for k in ("a", "u", "d1"))
        sigma = np.sum(Km * Bd * sd[None, :], 1) / sd
        G = dt(0.5) * (np.outer(a, a) - sd[:, None] * Bd * sd[None, :] + np.outer(u, d1) + np.outer(d1, u))
        per = [np.sum(G * Bm * ((x.astype(dt)[:, c:c + 1] - x.astype(dt)[None, :, c]) / dt(full_ls[c])) ** 2) for c in range(d)]
        g = [np.sum(G * Km) / dt(var)] + ([p / dt(full_ls[c]) for c, p in enumerate(per)] if ard else [sum(per) / dt(ls[0])])
        return {"K": Km, "matvec": Km @ t["vec"].astype(dt), "diag": sigma, "grad": np.array(g, dtype=dt)}

    hi, lo64 = host(LD), host(np.float64)
    out = {"K": (hi["K"], xr.tol(xr.abs_err(lo64["K"], hi["K"]), "K"), "abs")}
    for name in ("matvec", "diag", "grad"):
        out[name] = (hi[name], xr.tol(xr.rel_err(lo64[name], hi[name]), "dense_grad"), "rel")
    return out


# ---- the model cases ---------------------------------------------------------------------------------------------------------------
MODEL_CASES = [
    dict(name="probit_matern32_ard_129x3", lik="probit", kind="Matern32", n=129, d=3, ARD=True, variance=1.6, length_scales=[1.0, 0.8, 1.4],
         mean=None, seed=301),
    # rows 10 .. 19 repeat rows 0 .. 9: K is singular, Exp's cusp sits on the repeated pairs
    dict(name="logit_exp_65x2_repeats", lik="logit", kind="Exp", n=65, d=2, ARD=False, variance=1.4, length_scales=[1.1], mean=None,
         seed=303, repeat=True),
    # Periodic at d = 1 is positive semi-definite of rank 2 (cos(a - b) = cos a cos b + sin a sin b); the planted points
    dict(name="poisson_periodic_127x1", lik="poisson", kind="Periodic", n=127, d=1, ARD=False, variance=0.6, length_scales=[1.0], mean=None,
         seed=307, planted=True, offset=0.5, gain=0.8),
]


def model_inputs(case):
    """tests/_laplace_oracle.case_inputs with the case's own points: labels / counts drawn from a smooth latent of x."""
    import scipy.special
    import scipy.stats
    n, d, seed = case["n"], case["d"], case["seed"]
    x = rr.points(seed, n, d, case["length_scales"][0]) if case.get("planted") else rng.normal(seed, (n, d))
    if case.get("repeat"):
        x[10:20] = x[0:10]
    xc = np.clip(x, -4.0, 4.0)                                   # (the planted far row: a latent of ordinary size)
    g = np.sin(1.3 * xc[:, 0]) + 0.7 * np.cos(xc[:, 1:].sum(1)) + 0.3 * xc[:, 0]
    u = rng.uniform(seed + 1, n)
    if case["lik"] == "poisson":
        y = scipy.stats.poisson.ppf(u, np.exp(case["offset"] + case["gain"] * g))
    else:
        y = (u < (scipy.special.ndtr(1.5 * g) if case["lik"] == "probit" else scipy.special.expit(2.5 * g))).astype(np.float64)
    return {"x": x, "y": y.reshape(n, 1), "xs": rng.normal(seed + 2, (40, d))}


_ORACLES = {}


def oracle_numbers(case):
    """the long-double oracle's numbers and e64 = the fp64 oracle's distance from them (tests/golden/make_laplace_golden.py's
    model_case, computed here); B must be positive definite and the search converge in both arithmetics (it raises otherwise)."""
    if case["name"] not in _ORACLES:
        inp = model_inputs(case)
        o64 = lo.build_oracle(case, inp).search()
        old = lo.build_oracle(case, inp, dtype=lo.LD).search(until_stall=True)
        assert o64.steps <= 20 and old.steps <= 25, (o64.steps, old.steps)
        for o in (o64, old):                                     # the factor at the mode exists: B is positive definite there
            assert np.all(np.diag(o.L) > 0) and np.all(np.isfinite(np.asarray(o.f, dtype=np.float64)))
        res = {"loss": float(old.loss()), "e64": {"loss": xr.rel_err(o64.loss(), old.loss())}}
        g64, gld = o64.loss_grads(), old.loss_grads()
        res["e64"]["grad"] = max(xr.rel_err(a, b) for a, b in zip(g64[:2], gld[:2]))
        res["grad_variance"], res["grad_length_scales"] = (np.asarray(g, dtype=np.float64) for g in gld[:2])
        (m64, v64), (mld, vld) = o64.predict_f(inp["xs"]), old.predict_f(inp["xs"])
        c64, cld = o64.predict_f(inp["xs"], diag=False)[1], old.predict_f(inp["xs"], diag=False)[1]
        res["e64"].update(mean=xr.abs_err(m64, mld), var=xr.abs_err(v64, vld), cov=xr.abs_err(c64, cld))
        res["mean"], res["var"], res["cov"] = (np.asarray(t, dtype=np.float64) for t in (mld, vld, cld))
        res["inp"] = inp
        _ORACLES[case["name"]] = res
    return _ORACLES[case["name"]]


EP_DAMPING = 0.8
EP_CASES = [
    dict(name="ep_probit_exp_129x2", lik="probit", kind="Exp", n=129, d=2, ARD=False, variance=1.5, length_scales=[1.2], mean=None, seed=311,
         H=20),
    dict(name="ep_logit_matern32_ard_65x3", lik="logit", kind="Matern32", n=65, d=3, ARD=True, variance=2.0, length_scales=[1.1, 0.9, 1.5],
         mean=None, seed=313, H=32),
    dict(name="ep_probit_periodic_127x1", lik="probit", kind="Periodic", n=127, d=1, ARD=False, variance=1.2, length_scales=[1.0], mean=None,
         seed=317, planted=True, H=20),
]


def ep_numbers(case):
    """the long-double EP oracle's numbers and e64; the sweep must converge (not stall) in both arithmetics and B be positive
    definite at the fixed point (the oracle's Cholesky raises otherwise)."""
    from tests import _ep_oracle as eo
    if case["name"] not in _ORACLES:
        inp = model_inputs(case)
        o64 = eo.build_oracle(case, inp).search(damping=EP_DAMPING)
        old = eo.build_oracle(case, inp, dtype=eo.LD).search(damping=EP_DAMPING, until_stall=True)
        assert not o64.stalled and o64.sweeps <= 60, (case["name"], o64.sweeps, o64.stalled)
        for o in (o64, old):
            assert np.all(np.diag(o.L) > 0)
        res = {"sweeps": o64.sweeps, "loss": float(old.loss()), "e64": {"loss": xr.rel_err(o64.loss(), old.loss())}}
        g64, gld = o64.loss_grads(), old.loss_grads()
        res["e64"]["grad"] = max(xr.rel_err(a, b) for a, b in zip(g64[:2], gld[:2]))
        res["grad_variance"], res["grad_length_scales"] = (np.asarray(g, dtype=np.float64) for g in gld[:2])
        (m64, v64), (mld, vld) = o64.predict_f(inp["xs"]), old.predict_f(inp["xs"])
        res["e64"].update(mean=xr.abs_err(m64, mld), var=xr.abs_err(v64, vld))
        res["mean"], res["var"] = np.asarray(mld, dtype=np.float64), np.asarray(vld, dtype=np.float64)
        res["inp"] = inp
        _ORACLES[case["name"]] = res
    return _ORACLES[case["name"]]


def ep_golden(case):
    """the stored numbers of an EP case, with its inputs rebuilt."""
    from tests._util import load_npz
    g = load_npz(GOLDEN_NAME)
    meta = json.loads(str(g["meta"]))[case["name"]]
    res = dict(meta, inp=model_inputs(case))
    for key in ("grad_variance", "grad_length_scales", "mean", "var"):
        res[key] = g["%s__%s" % (case["name"], key)]
    return res
