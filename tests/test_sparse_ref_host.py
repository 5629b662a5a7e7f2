"""tests/_sparse_ref.py is checked here, on the host, before tests/test_gpu_sparse_xref.py lets it judge the native path:

  - every long-double gradient against central differences of the long-double bound and against fp64 autograd through the
    direct-difference oracle (two derivations that share nothing with the closed forms under test);
  - the bound and the predictions against the committed fp64 oracles (orc.VFEOracle, tests/_svgp_oracle.SVGPOracle);
  - the cap: on every case but the ladder one the derived tolerance xr.tol(e64, what) is no wider than the fixed tolerance the
    suite used so far for that quantity (1e-8 relative for the bound, 1e-7 relative for gradients, 1e-8 absolute for predictions);
  - resolving power: a reference evaluated WITH a planted mistake lies at least 100 tolerances from the true one.

Each test prints its figures (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

from oracle import gp_oracle as orc
from tests import _sparse_ref as sr
from tests import _svgp_oracle as so
from tests import _xref as xr
from tests._util import load_json

LD = xr.LD
CAP = {"loss": 1e-8, "grad": 1e-7, "mean": 1e-8, "var": 1e-8}
VFE = {c["name"]: c for c in sr.VFE_CASES}
SVGP = {c["name"]: c for c in sr.SVGP_CASES}


def _ids(cases):
    return [c["name"] for c in cases]


@functools.lru_cache(maxsize=None)
def inputs(fam, name):
    return sr.case_inputs((VFE if fam == "vfe" else SVGP)[name], svgp=fam == "svgp")


def host_jitter(case, inp):
    """the ladder case on the host: the jitter of the rung at which the fp64 factorisation of the direct-difference K(Z) succeeds,
    rung 0 at the least (two identical rows: without jitter a pivot is zero up to rounding, whatever a LAPACK makes of that).  The
    GPU test gives the reference the rung the native path reports instead."""
    if not case.get("ladder"):
        return 0.0
    d64 = sr.Direct64VFE(inp["x"], inp["y"], inp["z"], case["kernel"], case["noise"])
    with torch.no_grad():
        rung = max(0, orc.cholesky_rung(d64.K(d64.Z))[1])
    return 10.0 ** (-10 + rung)


def vfe_oracle(case, inp):
    k = case["kernel"]
    ls = np.asarray(k["length_scales"], dtype=np.float64) * (np.ones(case["d"]) if k.get("ARD") else 1.0)
    return orc.VFEOracle(inp["x"], inp["y"], inp["z"], k["kind"], k["variance"], ls, case["noise"])


@functools.lru_cache(maxsize=None)
def reference(fam, name):
    """what the GPU tests hold the native path to: dict(loss, grads, mean, var, cov, e64) -- the golden case from its fixture."""
    case, inp = (VFE if fam == "vfe" else SVGP)[name], inputs(fam, name)
    if case.get("golden"):
        g = {c["name"]: c for c in load_json("sparse_xref_cases.json")["cases"]}[name]
        return dict(loss=g["loss"], grads=g["grads"], mean=g["mean_pred"], var=g["var_pred"], cov=g["cov_pred"], e64=g["e64"])
    if fam == "svgp":
        return sr.svgp_reference(case, inp)
    return sr.vfe_reference(case, inp, jitter=host_jitter(case, inp))


# ---- gradients: central differences in long double ---------------------------------------------------------------------
# F(theta + t u) along one direction u per parameter block, Richardson-extrapolated central differences
#     D(h) = (F(h) - F(-h)) / 2h = F' + T h^2 + O(h^4),     D*(h) = (4 D(h) - D(2h)) / 3 = F' + T4 h^4 + ...
# The bound carries rounding eps_F ~ EPS_EFF |F| (EPS_EFF = 2^-63 sqrt(N M): long double sums of N M products), so D* carries
# ~ eps_F / h, which balances h^4 |F| at h = EPS_EFF^(1/5); both are then a small multiple of EPS_EFF^(4/5) |F|.  The truncation
# constant T4 is a fifth derivative along u, which for a direction in Z grows with every near pair of points; it is measured, not
# guessed: D*(2h) carries 16 T4 h^4, so |D*(h) - D*(2h)| is 15 times the truncation error of D*(h).
# Asserted: |g.u - D*(h)| <= 100 EPS_EFF^(4/5) max(1, |F|) + |D*(h) - D*(2h)|.
def _eps_eff(n, m):
    return 2.0 ** -63 * np.sqrt(n * m)


def _directions(theta, x, seed):
    """one random direction per block.  A row of Z with a training row or another inducing point within 1e-2 (hundreds of steps)
    stands still: at r = 0 Exp / Matern32 are not four times differentiable in Z, and in one dimension a step could carry the row
    across its neighbour, i.e. across Exp's cusp.  That covers the quarter of Z that sits ON training rows; those rows' gradient is
    held by the autograd check."""
    rs = np.random.RandomState(seed)
    out = {}
    for k, v in theta.items():
        u = rs.standard_normal(np.shape(v)).astype(LD)
        if k == "Z":
            z = np.asarray(v, dtype=np.float64)
            dx = np.sqrt(((z[:, None, :] - np.asarray(x)[None, :, :]) ** 2).sum(-1)).min(1)
            dz = np.sqrt(((z[:, None, :] - z[None, :, :]) ** 2).sum(-1)) + 1e9 * np.eye(z.shape[0])
            u[(dx < 1e-2) | (dz.min(1) < 1e-2)] = 0
            assert u.any()
        if k == "q_sqrt":
            u = np.tril(u)
        out[k] = u / max(1.0, float(np.sqrt(np.sum(u * u))))
    return out


def _kernel_of(case, th):
    k = dict(case["kernel"])
    k["variance"] = np.exp(th["variance"])[0]
    k["length_scales"] = np.exp(th["length_scales"])
    if k["kind"] == sr.COMPOSITE:
        k["linear_variance"], k["constant"] = np.exp(th["linear_variance"]), np.exp(th["constant"])[0]
    return k


def _theta(case, inp, mean, svgp):
    k, d = case["kernel"], case["d"]
    ls = xr.ld(k["length_scales"]) * (np.ones(d) if k.get("ARD") else np.ones(1))
    th = dict(variance=np.log(xr.ld([k["variance"]])), length_scales=np.log(ls), noise=np.log(xr.ld([case["noise"]])), mean=xr.ld(mean), Z=xr.ld(inp["z"]))
    if k["kind"] == sr.COMPOSITE:
        th.update(linear_variance=np.log(xr.ld(k["linear_variance"]) * np.ones(d)), constant=np.log(xr.ld([k["constant"]])))
    if svgp:
        S = xr.ld(inp["q_sqrt"])
        th.update(q_mu=xr.ld(inp["q_mu"]), q_sqrt=np.tril(S, -1) + np.diag(np.log(np.diag(S))))
    return th


def _build(case, inp, th, svgp):
    if not svgp:
        return sr.VFERef(inp["x"], inp["y"], th["Z"], _kernel_of(case, th), np.exp(th["noise"])[0], mean=th["mean"])
    i = slice(None) if inp["idx"] is None else inp["idx"]
    S = np.tril(th["q_sqrt"], -1) + np.diag(np.exp(np.diag(th["q_sqrt"])))
    return sr.SVGPRef(inp["x"][i], inp["y"][i], th["Z"], _kernel_of(case, th), np.exp(th["noise"])[0], th["q_mu"], S, mean=th["mean"],
                      num_data=case["n"])


FD_CASES = [("vfe", "one_chunk"), ("vfe", "m_across_a_leaf"), ("vfe", "composite"), ("svgp", "small"), ("svgp", "dy9"), ("svgp", "minibatch"),
            ("svgp", "composite")]


@pytest.mark.parametrize("fam,name", FD_CASES, ids=["%s-%s" % c for c in FD_CASES])
def test_gradients_against_central_differences(fam, name):
    """every block of the long-double gradient (a Constant mean included, VFE too) against central differences of the long-double
    bound along a random direction."""
    svgp = fam == "svgp"
    case, inp = (SVGP if svgp else VFE)[name], inputs(fam, name)
    mean = case.get("mean") or list(0.3 - 0.25 * np.arange(case["dy"]))
    th = _theta(case, inp, mean, svgp)
    ref = _build(case, inp, th, svgp)
    F, g = ref.loss(), ref.loss_grads()
    assert set(g) == set(th)
    eps = _eps_eff(ref.n, ref.m)
    h = LD(eps ** 0.2)
    bound = 100.0 * eps ** 0.8 * max(1.0, abs(float(F)))
    print("%s/%s: |F| %.3e  h %.2e  bound %.2e" % (fam, name, abs(float(F)), float(h), bound))
    for k, u in _directions(th, ref.X, 7).items():
        def along(t):
            return _build(case, inp, dict(th, **{k: th[k] + t * u}), svgp).loss()
        D = [(along(t * h) - along(-t * h)) / (2 * t * h) for t in (1, 2, 4)]
        Ds, Ds2 = (4 * D[0] - D[1]) / 3, (4 * D[1] - D[2]) / 3
        gu = np.sum(xr.ld(g[k]).reshape(u.shape) * u)
        err, trunc = abs(float(gu - Ds)), abs(float(Ds - Ds2))
        print("   d/d%-16s g.u %+.12e  central %+.12e  |diff| %.2e (%.1e of |g.u|; bound %.1e + %.1e)"
              % (k, float(gu), float(Ds), err, err / max(abs(float(gu)), 1e-300), bound, trunc))
        assert err <= bound + trunc, "%s: closed form %.15e, central differences %.15e, |diff| %.2e > %.2e" % (k, float(gu), float(Ds), err, bound + trunc)


NOISE_CASES = [("vfe", "m_across_a_leaf"), ("vfe", "composite"), ("svgp", "saved_vs_recompute"), ("svgp", "minibatch")]


@pytest.mark.parametrize("fam,name", NOISE_CASES, ids=["%s-%s" % c for c in NOISE_CASES])
def test_reference_does_not_depend_on_the_row_order(fam, name):
    """the same case with its rows permuted: only the order of the N-sized sums changes, so the distance between the two
    evaluations measures the reference's own rounding.  It has to vanish against the tolerances it is used with: 1e-13 relative
    for the bound and every gradient block, 1e-4 of the tightest floor (a gradient formed over Kuu^-1 and s Kuu + Kuf Kfu, right on
    paper, fails this at 1e-10: it subtracts terms cond(K(Z)) times the size of their difference)."""
    svgp = fam == "svgp"
    case, inp = (SVGP if svgp else VFE)[name], inputs(fam, name)
    i = np.arange(case["n"]) if inp["idx"] is None else inp["idx"]
    p = np.random.RandomState(5).permutation(len(i))
    refs = []
    for rows in (i, i[p]):
        x, y = inp["x"][rows], inp["y"][rows]
        refs.append(sr.SVGPRef(x, y, inp["z"], case["kernel"], case["noise"], inp["q_mu"], inp["q_sqrt"], mean=case.get("mean"), num_data=case["n"])
                    if svgp else sr.VFERef(x, y, inp["z"], case["kernel"], case["noise"]))
    d = {"loss": xr.rel_err(refs[1].loss(), refs[0].loss())}
    g0, g1 = refs[0].loss_grads(), refs[1].loss_grads()
    d.update({k: xr.rel_err(g1[k], g0[k]) for k in g0})
    print("%s/%s rows permuted: " % (fam, name) + "  ".join("%s %.1e" % kv for kv in d.items()))
    assert max(d.values()) <= 1e-13, d


ALL = [("vfe", c["name"]) for c in sr.VFE_CASES] + [("svgp", c["name"]) for c in sr.SVGP_CASES]
ALL_IDS = ["%s-%s" % c for c in ALL]


@pytest.mark.parametrize("fam,name", ALL, ids=ALL_IDS)
def test_gradients_against_fp64_autograd_and_the_cap(fam, name):
    """the long-double gradients against fp64 autograd through the direct-difference oracle: that distance IS e64["grads"], so it is
    held to the cap -- 16 e64 <= 1e-7 leaves the two derivations within 6.25e-9 relative of each other, every block -- and so are
    the tolerances of the loss and of the predictions.  The ladder case (two identical inducing points, K(Z) factored on a rung) is
    judged on the bound and predict_f alone; its tolerances are printed."""
    case, r = (VFE if fam == "vfe" else SVGP)[name], reference(fam, name)
    e = r["e64"]
    print("%s/%s" % (fam, name))
    for what in ("loss", "mean", "var"):
        print("   %-22s e64 %.2e  tol %.2e  cap %.0e" % (what, e[what], xr.tol(e[what], what), CAP[what]))
    for k, v in e["grads"].items():
        print("   d/d%-19s e64 %.2e  tol %.2e  cap %.0e" % (k, v, xr.tol(v, "grad"), CAP["grad"]))
    want = {"variance", "length_scales", "noise", "Z"} | ({"q_mu", "q_sqrt"} if fam == "svgp" else set()) \
        | ({"linear_variance", "constant"} if case["kernel"]["kind"] == sr.COMPOSITE else set())
    assert want <= set(e["grads"]) and want <= set(r["grads"])
    if case.get("ladder"):
        return
    for what in ("loss", "mean", "var"):
        assert xr.tol(e[what], what) <= CAP[what], (what, e[what])
    for k, v in e["grads"].items():
        assert xr.tol(v, "grad") <= CAP["grad"], (k, v)


# ---- the committed fp64 oracles ---------------------------------------------------------------------------------------
# Their own error: the Gram-trick distances r^2 = |a|^2 + |b|^2 - 2 a.b carry ~4 eps |x / ell|^2 of noise, which a smooth kind
# passes on as it is (well inside the suite's 1e-8) and Exp turns into sqrt(.) ~ 1e-7 in K next to a repeated point (tests/_xref.py);
# on top the bound carries cond(K(Z)) eps.  So: 1e-8 max(1, 1e-8 cond) relative for the bound, 1e-8 (Exp: 1e-6) absolute for
# predictions -- the figures tests/test_gpu_kinds_xref.py::test_vfe_exp holds the native path to against the same oracle.
def _oracle_tols(case, cond):
    exp = case["kernel"]["kind"] == "Exp"
    scale = max(1.0, 1e-8 * cond)
    return (1e-6 if exp else 1e-8) * scale, (1e-6 if exp else 1e-8) * scale


@pytest.mark.parametrize("name", [c["name"] for c in sr.VFE_CASES if c["kernel"]["kind"] != sr.COMPOSITE])
def test_vfe_reference_against_the_committed_oracle(name):
    """(orc.VFEOracle states stationary kinds only: the composite case is held by the autograd check above.)"""
    case, inp, r = VFE[name], inputs("vfe", name), reference("vfe", name)
    o = vfe_oracle(case, inp)
    jitter = host_jitter(case, inp)
    if jitter:                                                               # the oracle on the rung the reference was given
        base = o.K
        o.K = lambda a, b=None: base(a, b) + (jitter * torch.eye(a.shape[0], dtype=torch.float64) if b is None and a is o.Z else 0.0)
    with torch.no_grad():
        assert orc.cholesky_rung(o.K(o.Z))[1] == -1
        cond = float(torch.linalg.cond(o.K(o.Z)))
        elbo = o.log_likelihood().item()
        mu, var = o.predict_f(inp["xs"])
        _, cov = o.predict_f(inp["xs"], diag=False)
    tl, tp = _oracle_tols(case, cond)
    errs = (xr.rel_err(-elbo, r["loss"]), xr.abs_err(mu, r["mean"]), xr.abs_err(var, r["var"]), xr.abs_err(cov, r["cov"]))
    print("vfe/%s: cond K(Z) %.1e jitter %.0e  loss %.2e (tol %.1e)  mean %.2e var %.2e cov %.2e (tol %.1e)" % ((name, cond, jitter, errs[0], tl) + errs[1:] + (tp,)))
    assert errs[0] <= tl and max(errs[1:]) <= tp


@pytest.mark.parametrize("name", _ids(sr.SVGP_CASES))
def test_svgp_reference_against_the_committed_oracle(name):
    case, inp, r = SVGP[name], inputs("svgp", name), reference("svgp", name)
    o = so.SVGPOracle(inp["x"], inp["y"], inp["z"], case["kernel"], noise=case["noise"], q_mu=inp["q_mu"], q_sqrt=inp["q_sqrt"], mean=case.get("mean"))
    with torch.no_grad():
        cond = float(torch.linalg.cond(o.K(o.raw["Z"])))
        loss = o.loss(idx=inp["idx"]).item()
    mu, var = o.predict_f(inp["xs"])
    _, cov = o.predict_f(inp["xs"], diag=False)
    tl, tp = _oracle_tols(case, cond)
    errs = (xr.rel_err(loss, r["loss"]), xr.abs_err(mu, r["mean"]), xr.abs_err(var, np.asarray(r["var"], dtype=LD)[:, 0]), xr.abs_err(cov, r["cov"]))
    print("svgp/%s: cond K(Z) %.1e  loss %.2e (tol %.1e)  mean %.2e var %.2e cov %.2e (tol %.1e)" % ((name, cond, errs[0], tl) + errs[1:] + (tp,)))
    assert errs[0] <= tl and max(errs[1:]) <= tp


# ---- resolving power ---------------------------------------------------------------------------------------------------
def _distance(planted, true, e64, xs, quantities):
    """{quantity: distance of the planted reference from the true one, in tolerances of that quantity} -- "grad": the block that
    moves the most, each in its own tolerance."""
    out = {}
    if "loss" in quantities:
        out["loss"] = xr.rel_err(planted.loss(), true["loss"]) / xr.tol(e64["loss"], "loss")
    if "grad" in quantities:
        g = planted.loss_grads()
        out["grad"] = max(xr.rel_err(g[k], true["grads"][k]) / xr.tol(e64["grads"][k], "grad") for k in true["grads"])
        for k in quantities:
            if k.startswith("grad:"):
                out[k] = xr.rel_err(g[k[5:]], true["grads"][k[5:]]) / xr.tol(e64["grads"][k[5:]], "grad")
    if "mean" in quantities:
        mu, var = planted.predict_f(xs, True)
        out["mean"] = xr.abs_err(mu, true["mean"]) / xr.tol(e64["mean"], "mean")
        out["var"] = xr.abs_err(var, true["var"]) / xr.tol(e64["var"], "var")
    return out


# (family, case, mistake, where, the quantities of the GPU check that the mistake can reach)
PLANTS = [
    ("vfe", "ragged_multi_chunk", "drop_last_row", 0, ("loss", "grad", "mean")),               # mean: predict_f's mean AND variance
    ("vfe", "short_k_slices", "drop_k_slice", 1280, ("loss", "grad", "mean")),                 # the last 16 columns of chunk 3's 276 + pad
    ("vfe", "ragged_multi_chunk", "trkff_one_chunk", 256, ("loss", "grad", "grad:variance", "grad:noise")),   # (no part in predict_f)
    ("vfe", "ragged_multi_chunk", "gq_triangle", 0, ("grad", "grad:variance", "grad:length_scales", "grad:Z")),
    ("svgp", "minibatch", "scale_one", 0, ("loss", "grad", "grad:noise", "grad:q_mu")),
    ("svgp", "saved_vs_recompute", "gq_triangle", 0, ("grad", "grad:Z", "grad:q_sqrt")),
    ("svgp", "dy9", "drop_kd_diag", 0, ("grad", "grad:q_sqrt")),
]


@pytest.mark.parametrize("fam,name,plant,at,quantities", PLANTS, ids=["%s-%s-%s" % p[:3] for p in PLANTS])
def test_resolving_power(fam, name, plant, at, quantities):
    """a reference evaluated with the mistake planted lies at least 100 tolerances from the true one, in every quantity of the GPU
    check that the mistake can reach (a mistake in the backward alone leaves the loss and the predictions where they are)."""
    case, inp, true = (VFE if fam == "vfe" else SVGP)[name], inputs(fam, name), reference(fam, name)
    if fam == "vfe":
        planted = sr.vfe_refs(case, inp, plant=plant, plant_at=at)[0]
    else:
        planted = sr.svgp_refs(case, inp, plant=plant)[0]
    d = _distance(planted, true, true["e64"], inp["xs"], quantities)
    print("%s/%s with %s: " % (fam, name, plant) + "  ".join("%s %.1e tol" % kv for kv in d.items()))
    assert all(v >= 100.0 for v in d.values()), d
