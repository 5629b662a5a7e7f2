"""The streamed VFE bound, the SVGP bound, their closed-form backwards and their predictions (gptorch_amd/models/sparse_gpr.py)
against the long-double statements of tests/_sparse_ref.py, on every route the module's switches select -- at the smallest
shapes that cross each switch's edge -- and the three reductions behind the bounds' scalars (csrc/matutil.hip) through the C ABI
against long-double sums.

Tolerances are tests/_xref.tol: max(16 e64, FLOOR[what]), e64 the distance of the plain fp64 CPU evaluation of the same quantity
(tests/_sparse_ref.Direct64VFE / Direct64SVGP) from the long-double one; tests/test_sparse_ref_host.py holds every one of them
under the fixed tolerance the suite used before, and checks the reference itself.  Loss and gradients are relative to
max(1, |reference|) (xr.rel_err), predictions absolute.  The module's switches are set with monkeypatch.setattr: their
environment variables are read once, at import.  Every check prints achieved error against tolerance (pytest -s).

Measured on an MI355X (achieved / tolerance; "grad": the parameter block with the least margin).  Except for the inverse form and
the ladder case 16 e64 is below the floors, so those are the tolerances: 1e-10 loss, 1e-9 gradients, 1e-10 predictions.

    case (knobs)                                  loss            gradient, least margin                 mean      var
    vfe one_chunk                                 2.4e-16         2.3e-14  Z                             2.1e-15   4.8e-16
    vfe m_across_a_leaf                           2.0e-15         2.1e-12  Z                             1.5e-14   4.1e-15
    vfe ragged_multi_chunk (LANES 1 and 2)        4.7e-15         1.5e-12  Z                             1.2e-14   9.6e-15
    vfe exact_multiple                            5.9e-16         3.4e-13  Z                             3.3e-15   1.8e-15
    vfe short_k_slices (128 / 0)                  4.5e-16         3.0e-12 / 2.3e-12  Z                   1.6e-14   2.4e-15
    vfe split_k_tail                              1.0e-15         6.6e-13  Z                             4.2e-14   2.1e-15
    vfe split_k_miss (one chunk / 8192 + 8)       3.2e-15         1.7e-12 / 2.0e-12  Z                   6.7e-14   1.5e-15
    vfe inverse_form                              3.6e-13/1.5e-10 1.2e-10  kernel.variance (8x)          1.1e-12   3.5e-13
    vfe blocked_one_block                         6.5e-16         7.7e-13  Z                             1.1e-14   2.1e-15
    vfe blocked_two_blocks                        5.9e-15         1.4e-10  Z (7x)                        1.3e-13   4.5e-15
    vfe composite                                 6.7e-15         8.1e-10  Constant's variance (1.2x)    4.7e-14   2.6e-14
    vfe ladder (rung 0)                           4.6e-10/2.1e-9  (not judged)                           2.1e-11   9.8e-11/5.1e-10
    svgp small                                    6.8e-16         9.1e-14  kernel.length_scales          1.5e-15   1.7e-15
    svgp dy9                                      1.2e-16         8.1e-15  kernel.length_scales          8.6e-15   4.0e-15
    svgp saved_vs_recompute (one / six chunks)    5.5e-13         3.1e-12 / 2.4e-12                      2.1e-12   2.2e-12
    svgp minibatch                                7.5e-13         1.2e-10  kernel.variance (8x)          2.9e-12   2.1e-12
    svgp composite                                3.4e-14         1.0e-11  Constant's variance           5.0e-14   1.5e-13

One route has less than twice its tolerance in hand: the VFE composite case's gradient w.r.t. the Constant leaf's variance, a sum of
all of dF/dKuu and dF/dKuf that comes to 2.15 (the Linear leaf's: 5x).  The backward forms dF/dKuf as P Kuf with the explicit
P = L^-T [..] L^-1 (cond K(Z) = 2.4e5 here, max |P| = 2.8e3): the products |P| |Kuf| behind that sum add up to 1.1e7, so fp64
rounding alone allows ~1e-9 there, and the floor it is held to is relative to max(1, 2.15), not to the size of those terms."""
import functools

import numpy as np
import pytest
import torch

import gptorch_amd
from gptorch_amd import _ops, likelihoods
from gptorch_amd.models import VFE, sparse_gpr
from tests import _sparse_ref as sr
from tests import _svgp_oracle as so
from tests import _xref as xr
from tests._util import load_json

pytestmark = pytest.mark.gpu

LD = xr.LD
KNOBS = ("CHUNK_ROWS", "LANES", "SPLIT_K", "SYRK_K_SLICE", "INVERSE_MIN_M", "INVERSE_BLOCK", "BLOCKED_SOLVE_MIN_M")


@functools.lru_cache(maxsize=None)
def inputs(fam, name):
    return sr.case_inputs({c["name"]: c for c in (sr.VFE_CASES if fam == "vfe" else sr.SVGP_CASES)}[name], svgp=fam == "svgp")


@functools.lru_cache(maxsize=None)
def reference(fam, name, jitter=0.0):
    """computed once per module and left as it is; the case that is too large for that comes from its fixture
    (tests/golden/make_sparse_xref_golden.py)."""
    case = {c["name"]: c for c in (sr.VFE_CASES if fam == "vfe" else sr.SVGP_CASES)}[name]
    if case.get("golden"):
        g = {c["name"]: c for c in load_json("sparse_xref_cases.json")["cases"]}[name]
        assert all(g[k] == case[k] for k in ("n", "m", "d", "dy", "kernel", "noise", "seed"))
        return dict(loss=g["loss"], grads=g["grads"], mean=g["mean_pred"], var=g["var_pred"], cov=g["cov_pred"], e64=g["e64"])
    inp = inputs(fam, name)
    return sr.vfe_reference(case, inp, jitter) if fam == "vfe" else sr.svgp_reference(case, inp)


def check_loss(tag, loss, ref):
    err, tol = xr.rel_err(loss.item(), ref["loss"]), xr.tol(ref["e64"]["loss"], "loss")
    print("%s: loss %.12f reference %.12f rel err %.2e (tol %.1e, margin %.1fx)" % (tag, loss.item(), float(ref["loss"]), err, tol, tol / max(err, 1e-300)))
    assert loss.dim() == 0 and loss.is_cuda
    assert err <= tol


def check_grads(model, names, ref):
    params = dict(model.named_parameters())
    for on, mn in names.items():
        got = params[mn].grad.detach().cpu().numpy()
        want = np.asarray(ref["grads"][on], dtype=LD).reshape(got.shape)
        err, tol = xr.rel_err(got, want), xr.tol(ref["e64"]["grads"][on], "grad")
        print("   d/d%-32s rel err %.2e of max %.2e (tol %.1e, margin %.1fx)" % (mn, err, float(np.max(np.abs(want))), tol, tol / max(err, 1e-300)))
        assert err <= tol, mn


def check_predictions(model, inp, ref, noise):
    xs = torch.tensor(inp["xs"]).cuda()
    e = ref["e64"]
    mu, var = model.predict_f(xs)
    mu2, cov = model.predict_f(xs, diag=False)
    _, vy = model.predict_y(xs)
    want_var = np.asarray(ref["var"], dtype=LD)
    errs = (xr.abs_err(mu, ref["mean"]), xr.abs_err(mu2, ref["mean"]), xr.abs_err(var, want_var), xr.abs_err(cov, ref["cov"]),
            xr.abs_err(vy, want_var + LD(noise)))
    tm, tv = xr.tol(e["mean"], "mean"), xr.tol(e["var"], "var")
    print("   predict_f: mean %.2e / %.2e (tol %.1e)  var %.2e cov %.2e  predict_y var %.2e (tol %.1e)" % (errs[0], errs[1], tm, errs[2], errs[3], errs[4], tv))
    assert tuple(var.shape) == tuple(mu.shape) == np.shape(ref["mean"])
    assert max(errs[:2]) <= tm and max(errs[2:]) <= tv


# ---- VFE ---------------------------------------------------------------------------------------------------------------
def vfe_model(case, inp):
    k, d = case["kernel"], case["d"]
    if k["kind"] == sr.COMPOSITE:
        kern = gptorch_amd.kernels.Linear(d, variance=k["linear_variance"]) \
            + gptorch_amd.kernels.Rbf(d, variance=k["variance"], length_scales=k["length_scales"]) + gptorch_amd.kernels.Constant(d, variance=k["constant"])
    else:
        ls = np.asarray(k["length_scales"], dtype=np.float64) * (np.ones(d) if k.get("ARD") else 1.0)
        kern = getattr(gptorch_amd.kernels, k["kind"])(d, variance=k["variance"], length_scales=ls, ARD=bool(k.get("ARD")))
    m = VFE(inp["x"], inp["y"], kern, inducing_points=inp["z"].copy(), likelihood=likelihoods.Gaussian(variance=case["noise"]))
    m.cuda()
    return m


def vfe_names(case):
    return {k: v for k, v in so.model_names(case).items() if not k.startswith("q_")}


def assert_route(case, knobs):
    """the run takes the route the case is there for."""
    n, m = case["n"], case["m"]
    nc = sparse_gpr._chunk_rows(n)
    sizes = [r for _, r in sparse_gpr._chunks(n, nc)]
    if "chunks" in case:
        assert sizes == case["chunks"], sizes
    if not knobs:
        assert sizes == [n]
    assert sparse_gpr._blocked_solve(m, n) == ("BLOCKED_SOLVE_MIN_M" in knobs)
    assert (m >= sparse_gpr.INVERSE_MIN_M and n >= 4 * m) == ("INVERSE_MIN_M" in knobs)
    if "SPLIT_K" in knobs:                                                   # _stream_gram: split > 1
        assert nc >= 4096 * sparse_gpr.SPLIT_K and sparse_gpr.SPLIT_K > 1
        missed = [r for r in sizes if _ops.round_up(r, 16) % (16 * sparse_gpr.SPLIT_K)]
        assert missed == {"split_k_tail": [400], "split_k_miss": [8200] if len(sizes) == 1 else [8]}[case["name"]]
    else:
        assert nc < 4096 * sparse_gpr.SPLIT_K
    if "SYRK_K_SLICE" in knobs and knobs["SYRK_K_SLICE"]:                      # a last slice shorter than the others
        assert any(_ops.round_up(r, 16) % knobs["SYRK_K_SLICE"] for r in sizes)


@pytest.mark.parametrize("case", [c for c in sr.VFE_CASES if not c.get("ladder")], ids=[c["name"] for c in sr.VFE_CASES if not c.get("ladder")])
def test_vfe(device, monkeypatch, case):
    """loss, every parameter gradient (Z included), predict_f (diag and full) and predict_y's variance, once per knob set of the case,
    each against the one reference of the case."""
    inp, ref = inputs("vfe", case["name"]), reference("vfe", case["name"])
    for knobs in case["knobs"]:
        with monkeypatch.context() as mp:
            for k, v in knobs.items():
                assert k in KNOBS
                mp.setattr(sparse_gpr, k, v)
            assert_route(case, knobs)
            m = vfe_model(case, inp)
            loss = m.loss()
            loss.backward()
            check_loss("vfe/%s %s" % (case["name"], knobs or "defaults"), loss, ref)
            check_grads(m, vfe_names(case), ref)
            check_predictions(m, inp, ref, case["noise"])


def test_vfe_ladder(device):
    """two identical inducing points: K(Z) is singular, the native factorisation climbs the jitter ladder and reports its rung; the
    reference is given that jitter, 10^(-10 + rung).  The bound and predict_f are judged, at tolerances that are printed: at
    cond K(Z) ~ 1e11 they are the only ones of this module above their floors.  The gradients are printed against theirs."""
    case = {c["name"]: c for c in sr.VFE_CASES}["ladder"]
    inp = inputs("vfe", "ladder")
    assert np.array_equal(inp["z"][-1], inp["z"][-2])
    m = vfe_model(case, inp)
    loss = m.loss()
    loss.backward()
    rung = m._bound(m.X)[1].f_uu.jitter_rung
    print("vfe/ladder: rung %d" % rung)
    assert rung >= 0
    ref = reference("vfe", "ladder", 10.0 ** (-10 + rung))
    check_loss("vfe/ladder", loss, ref)
    check_predictions(m, inp, ref, case["noise"])
    params = dict(m.named_parameters())
    for on, mn in vfe_names(case).items():
        print("   (not judged) d/d%-19s rel err %.2e (tol %.1e)" % (mn, xr.rel_err(params[mn].grad.cpu().numpy(), np.asarray(ref["grads"][on], dtype=LD).reshape(params[mn].shape)),
                                                              xr.tol(ref["e64"]["grads"][on], "grad")))


# ---- SVGP --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sr.SVGP_CASES, ids=[c["name"] for c in sr.SVGP_CASES])
def test_svgp(device, monkeypatch, case):
    """the bound (a fixed, gathered index set where the case has one), every parameter gradient (Z, q_mu, q_sqrt and the mean
    included), predict_f and predict_y's variance, once per knob set; two knob sets (the single chunk whose (At, T) the backward
    starts from, and six chunks with a tail that it recomputes) also agree with each other within the same tolerances."""
    inp, ref = inputs("svgp", case["name"]), reference("svgp", case["name"])
    names, runs = so.model_names(case), []
    for knobs in case["knobs"]:
        with monkeypatch.context() as mp:
            for k, v in knobs.items():
                assert k in KNOBS
                mp.setattr(sparse_gpr, k, v)
            rows = case["n"] if inp["idx"] is None else len(inp["idx"])
            sizes = [r for _, r in sparse_gpr._chunks(rows, sparse_gpr._chunk_rows(rows))]
            if case["name"] == "saved_vs_recompute":
                assert sizes == ([1300] if not knobs else [256] * 5 + [20])
            m = so.build_model(gptorch_amd, case, inp)
            m.cuda()
            if inp["idx"] is None:
                loss = m.loss()
            else:
                i = torch.as_tensor(inp["idx"], device=m.X.device)
                assert rows == case["nb"] < case["n"] and bool((i[1:] - i[:-1] > 1).any())        # gathered, not a slice
                loss = m.loss(x=m.X[i], y=m.Y[i])
            loss.backward()
            check_loss("svgp/%s %s" % (case["name"], knobs or "defaults"), loss, ref)
            check_grads(m, names, ref)
            check_predictions(m, inp, ref, case["noise"])
            runs.append((loss.item(), {mn: dict(m.named_parameters())[mn].grad.detach().cpu().numpy().copy() for mn in names.values()}))
    for (la, ga), (lb, gb) in zip(runs, runs[1:]):
        assert xr.rel_err(la, lb) <= xr.tol(ref["e64"]["loss"], "loss")
        for on, mn in names.items():
            err = xr.rel_err(ga[mn], gb[mn])
            print("   saved against recomputed d/d%-24s rel diff %.2e" % (mn, err))
            assert err <= xr.tol(ref["e64"]["grads"][on], "grad"), mn


# ---- the three reductions behind the bounds' scalars, through the C ABI ------------------------------------------------------
# Tolerance: 16 x the error of a plain fp64 numpy evaluation of the same sum against its long-double value, floored at
# 64 * 2^-53 * sum |terms|.
def _sum_tol(v64, v_ld, abs_terms):
    return max(16.0 * abs(float(LD(v64) - v_ld)), 64.0 * 2.0 ** -53 * float(abs_terms))


def _lib():
    return _ops._native.lib()


def _dot2d(x, ldx, sx, y, ldy, sy, rows, cols, batch):
    return _ops.dot2d_raw(_ops._ptr(x), ldx, sx, None if y is None else _ops._ptr(y), ldy, sy, rows, cols, batch, x.device).cpu().numpy()


@pytest.mark.parametrize("with_y", [False, True], ids=["sum", "dot"])
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 255), (1, 256), (1, 257), (3, 171), (130, 9)])
def test_dot2d_batched(device, rows, cols, with_y):
    """gpn_dot2d_batched: padded ldx / ldy with the padding (and everything between the problems) poisoned with NaN, y NULL and
    non-NULL, three problems at a stride -- each value bit-identical to the same problem launched alone."""
    rs = np.random.RandomState(1000 * rows + cols)
    ldx, ldy, batch = cols + 3, cols + 5, 3
    sx, sy = rows * ldx + 7, rows * ldy + 11
    xb, yb = np.full(batch * sx, np.nan), np.full(batch * sy, np.nan)
    xs = rs.standard_normal((batch, rows, cols)) * np.exp(rs.uniform(-3, 3, (batch, rows, cols)))
    ys = rs.standard_normal((batch, rows, cols))
    for z in range(batch):
        xb[z * sx: z * sx + rows * ldx].reshape(rows, ldx)[:, :cols] = xs[z]
        yb[z * sy: z * sy + rows * ldy].reshape(rows, ldy)[:, :cols] = ys[z]
    xd, yd = torch.tensor(xb).cuda(), (torch.tensor(yb).cuda() if with_y else None)
    got = _dot2d(xd, ldx, sx, yd, ldy, sy, rows, cols, batch)
    for z in range(batch):
        terms = xs[z].astype(LD) * (ys[z].astype(LD) if with_y else LD(1))
        want = np.sum(terms)
        tol = _sum_tol(np.sum(xs[z] * ys[z]) if with_y else np.sum(xs[z]), want, np.sum(np.abs(terms)))
        err = abs(float(LD(got[z]) - want))
        print("dot2d %dx%d y=%s problem %d: err %.2e tol %.2e" % (rows, cols, with_y, z, err, tol))
        assert err <= tol
        alone = _dot2d(xd[z * sx:], ldx, 0, None if yd is None else yd[z * sy:], ldy, 0, rows, cols, 1)
        assert alone[0] == got[z] and not np.isnan(got[z])


@pytest.mark.parametrize("e", [0, 1, 3])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 8193])
def test_lml_reduce_batched(device, n, e):
    """gpn_lml_reduce_batched: three factor buffers at a stride, only the diagonal and the e extra rows are meant to be read --
    everything else is NaN --, bit-identical per problem to gpn_lml_reduce; out3 = (sum log L_ii, sum of squares of the extra rows,
    -0.5 quad - e logdet - 0.5 e n log(2 pi)) against long-double values."""
    rs = np.random.RandomState(10 * n + e)
    lda, batch = n + 3, 3
    sA = (n + e) * lda + 5
    A = torch.full((batch * sA,), float("nan"), dtype=torch.float64, device="cuda")
    diag = np.exp(rs.uniform(-2, 2, (batch, n)))
    extra = rs.standard_normal((batch, e, n))
    for z in range(batch):
        A[z * sA: z * sA + n * lda][::lda + 1] = torch.tensor(diag[z]).cuda()
        if e:
            A[z * sA + n * lda: z * sA + (n + e) * lda].view(e, lda)[:, :n] = torch.tensor(extra[z]).cuda()
    out = torch.empty(batch, 3, dtype=torch.float64, device="cuda")
    _ops._native.check(_lib().gpn_lml_reduce_batched(_ops._stream(A.device), _ops._ptr(A), n, e, lda, sA, _ops._ptr(out), batch), "gpn_lml_reduce_batched")
    got = out.cpu().numpy()
    for z in range(batch):
        logs, sq = np.log(diag[z].astype(LD)), extra[z].astype(LD) ** 2
        logdet, quad = np.sum(logs), np.sum(sq)
        third = -LD(0.5) * quad - e * logdet - LD(0.5) * e * n * np.log(2 * LD(np.pi))
        l64, q64 = np.sum(np.log(diag[z])), np.sum(extra[z] ** 2)
        t64 = -0.5 * q64 - e * l64 - 0.5 * e * n * np.log(2 * np.pi)
        tols = (_sum_tol(l64, logdet, np.sum(np.abs(logs))), _sum_tol(q64, quad, quad),
                _sum_tol(t64, third, LD(0.5) * quad + e * np.sum(np.abs(logs)) + LD(0.5) * e * n * np.log(2 * LD(np.pi))))
        errs = [abs(float(LD(g) - w)) for g, w in zip(got[z], (logdet, quad, third))]
        print("lml_reduce n=%d e=%d problem %d: errs %s tols %s" % (n, e, z, ["%.2e" % v for v in errs], ["%.2e" % v for v in tols]))
        assert all(a <= t for a, t in zip(errs, tols))
        one = torch.empty(3, dtype=torch.float64, device="cuda")
        _ops._native.check(_lib().gpn_lml_reduce(_ops._stream(A.device), _ops._ptr(A[z * sA:]), n, e, lda, _ops._ptr(one)), "gpn_lml_reduce")
        assert np.array_equal(one.cpu().numpy(), got[z])


@pytest.mark.parametrize("cols", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("rows", [1, 17])
def test_row_sumsq(device, rows, cols):
    """gpn_row_sumsq with a padded lda, the padding NaN."""
    rs = np.random.RandomState(100 * rows + cols)
    lda = cols + 5
    a = rs.standard_normal((rows, cols)) * np.exp(rs.uniform(-3, 3, (rows, cols)))
    buf = np.full((rows, lda), np.nan)
    buf[:, :cols] = a
    got = _ops.row_sumsq(torch.tensor(buf).cuda(), rows, cols).cpu().numpy()
    for r in range(rows):
        sq = a[r].astype(LD) ** 2
        want = np.sum(sq)
        tol = _sum_tol(np.sum(a[r] * a[r]), want, want)
        err = abs(float(LD(got[r]) - want))
        print("row_sumsq %dx%d row %d: err %.2e tol %.2e" % (rows, cols, r, err, tol))
        assert err <= tol
