"""The refinement step of the LML's quadratic form (csrc/refine.hip, csrc/refine_tail.h) kernel by kernel against the references of
tests/_refine_ref.py: the back-substitution gpn_backsub (persistent and stepwise form, lock-step form) against long-double
substitution with the native factor; the residual pass over the stationary kinds against the long-double product of the assembled
matrix, within that product's own error bound; the composed step gpn_lml_refine / gpn_lml_refine_dense at small sizes, pinned on
its own intermediates in exact arithmetic; gpn_refine_finish against exact rational arithmetic on inputs that cancel; and
gpn_gemv_t_acc.  The double-double kernels are held to bounds that a plain fp64 evaluation of the same quantity misses: each test
asserts that negative control on its own inputs before it looks at the kernel's output (tests/test_refine_ref_host.py shows the
same controls without a GPU).  Every test prints one "XREF refine ..." line with its worst err / tol.

Work buffers have exactly the size the library asks for and are poisoned with NaN; outputs are pre-filled, and what the entry
point must not write is checked to be untouched."""
import ctypes

import numpy as np
import pytest
import torch

from gptorch_amd import _native, _ops
from gptorch_amd._ops import _ptr, _stream
from oracle import gp_oracle as orc
from tests import _factor_ref as fr
from tests import _refine_ref as rr
from tests import _xref as xr
from tests.test_gpu_factor_xref import load

pytestmark = pytest.mark.gpu

LD = xr.LD
NAN = float("nan")
SENTINEL = -7.25e300                  # what an entry point must leave alone: no computed value


def _t(a, device):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=device)


def _full(shape, value, device):
    return torch.full(shape, value, dtype=torch.float64, device=device)


def _work(nbytes, device):
    """a work buffer of exactly nbytes, NaN in every word"""
    nbytes = int(nbytes)
    assert nbytes > 0 and nbytes % 8 == 0
    return _full((nbytes // 8,), NAN, device)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def report(what, ident, pairs, extra=""):
    """pairs: (label, err, tol) -> prints the worst err / tol and asserts every one"""
    worst = max(pairs, key=lambda p: p[1] / p[2])
    print("XREF refine %s %s worst %s err/tol %.3g (err %.3g)%s" % (what, ident, worst[0], worst[1] / worst[2], worst[1], extra))
    for label, err, t in pairs:
        assert err <= t, (what, ident, label, "err %.3g tol %.3g" % (err, t))


# ---------------------------------------------------------------------------------------------------------------------
# (a) back-substitution
# ---------------------------------------------------------------------------------------------------------------------
def _factor(family, n, dy, device, seed=0, f=None):
    """the shipped driver's factor of (family, n) with dy right-hand sides riding along -> (Factor, sqrt(a_ii))"""
    A = fr.matrix(family, n, seed)
    f = _ops.Factor(n, dy, device) if f is None else f
    load(f, A, fr.rhs(A, dy, seed))
    assert f.potrf() == 0
    return f, np.sqrt(np.diag(A))


def _backsub(f):
    """gpn_backsub through the ABI: work of exactly gpn_backsub_work_bytes (NaN), out [dy, n + 3] pre-filled -> out as numpy"""
    lib = _native.lib()
    n, dy = f.n, f.e
    work = _work(lib.gpn_backsub_work_bytes(n, dy), f.device)
    out = _full((dy, n + 3), SENTINEL, f.device)
    st = lib.gpn_backsub(_stream(f.device), _ptr(f.A), f.ld, _ptr(f.winv), n, dy, _ptr(work), _ptr(out), n + 3)
    _native.check(st, "gpn_backsub")
    out = out.cpu().numpy()
    assert np.all(out[:, n:] == SENTINEL)
    return out[:, :n].copy()


def _backsub_pair(f, sd):
    """(err, tol) of a back-substitution result against long-double substitution with the native L and alpha"""
    L, alpha = f.lower().cpu().numpy(), f.extra().cpu().numpy().copy()
    ref = rr.backsub_ref(L, alpha)
    tol = fr.tol(rr.backsub_e64(L, alpha, ref, sd))
    return lambda a: (rr.backsub_metric(a, ref, sd), tol)


@pytest.mark.parametrize("family,n,dy", rr.backsub_cases(), ids=["%s-%d-%d" % c for c in rr.backsub_cases()])
def test_backsub_against_long_double(device, family, n, dy):
    """gpn_backsub (the persistent form): L^-T alpha against long-double substitution with the SAME native L and alpha, rows weighed
    by sqrt(a_ii); n < 128, full and ragged last blocks, one to nine blocks; dy = 1 (<1>), 2 (one <RDY> pass), 3 (a ragged second
    pass), 5 (three passes).  Nothing right of column n of `out` is written; two calls give the same bits."""
    f, sd = _factor(family, n, dy, device)
    judge = _backsub_pair(f, sd)
    a = _backsub(f)
    assert not np.isnan(a).any()
    assert np.array_equal(_bits(_backsub(f)), _bits(a))
    err, tol = judge(a)
    report("backsub", "%s-%d-%d" % (family, n, dy), [("persistent", err, tol)], " = %.1f u" % (err / fr.U))


@pytest.mark.parametrize("dy", rr.BACKSUB_DY)
@pytest.mark.parametrize("n", rr.BACKSUB_STEPWISE_N)
def test_backsub_stepwise_form(device, n, dy):
    """the one-launch-per-block form (tools' build switch) below the sizes tests/test_gpu_refine_backsub.py covers: the bits of
    the persistent form, and the same tolerance."""
    lib = _native.debug_begin()
    try:
        lib.gpn_debug_set_backsub_persistent.restype = ctypes.c_int
        lib.gpn_debug_set_backsub_persistent.argtypes = [ctypes.c_int]
        f, sd = _factor("well", n, dy, device)
        judge = _backsub_pair(f, sd)
        lib.gpn_debug_set_backsub_persistent(0)
        step = _backsub(f)
        lib.gpn_debug_set_backsub_persistent(1)
        pers = _backsub(f)
    finally:
        lib.gpn_debug_set_backsub_persistent(1)
        _native.debug_end()
    assert np.array_equal(_bits(step), _bits(pers))
    err, tol = judge(step)
    report("backsub_stepwise", "well-%d-%d" % (n, dy), [("stepwise", err, tol)], " = %.1f u; bits of the persistent form" % (err / fr.U))


@pytest.mark.parametrize("n,dy", rr.BACKSUB_BATCHED)
def test_backsub_batched(device, n, dy):
    """gpn_backsub_batched over three factors: every slot is bit-identical to its single call (and so within its tolerance), and
    nothing right of column n is written."""
    lib = _native.lib()
    B = 3
    fb = _ops.FactorBatch(B, n, dy, device)
    single, pairs = [], []
    for b in range(B):
        f, sd = _factor("well", n, dy, device, seed=b, f=fb.factor(b))
        a = _backsub(f)
        pairs.append(("slot %d" % b,) + _backsub_pair(f, sd)(a))
        single.append(a)
    ldo = n + 3
    work = _work(lib.gpn_backsub_batched_work_bytes(n, dy, B), device)
    out = _full((B, dy, ldo), SENTINEL, device)
    st = lib.gpn_backsub_batched(_stream(device), B, _ptr(fb.A), fb.ld, fb.sA, _ptr(fb.winv), fb.sW, n, dy, _ptr(work), _ptr(out), ldo, dy * ldo)
    _native.check(st, "gpn_backsub_batched")
    out = out.cpu().numpy()
    assert np.all(out[:, :, n:] == SENTINEL)
    for b in range(B):
        assert np.array_equal(_bits(out[b, :, :n]), _bits(single[b])), b
    report("backsub_batched", "%d-%d" % (n, dy), pairs, "; every slot the bits of its single call")


# ---------------------------------------------------------------------------------------------------------------------
# (b) residual pass over the stationary kinds
# ---------------------------------------------------------------------------------------------------------------------
def _resid_part(kind, X, var, ls, nz, a, q0, q1):
    """gpn_refine_resid_part -> ka [dy, lds, 2] as numpy (rows >= n: the NaN it was filled with)"""
    lib = _native.lib()
    n, d = X.shape
    dy, lds = a.shape
    ka = _full((dy, lds, 2), NAN, X.device)
    nbytes = int(lib.gpn_refine_resid_part_work_bytes(dy, q1 - q0))
    assert (nbytes == 0) == (q1 == q0)
    work = _work(max(nbytes, 8), X.device)                     # (an empty tile range needs no scratch, but a pointer)
    st = lib.gpn_refine_resid_part(_stream(X.device), _ops.KINDS[kind], _ptr(X), n, d, _ptr(var), _ptr(ls), ls.numel(), _ptr(nz), _ptr(a), dy,
                                   q0, q1, _ptr(work), _ptr(ka))
    _native.check(st, "gpn_refine_resid_part")
    ka = ka.cpu().numpy()
    assert np.isnan(ka[:, n:]).all() and not np.isnan(ka[:, :n]).any()
    return ka[:, :n]


def _assembled(kind, X, var, ls, noise):
    """Kyy as gpn_kernel_matrix assembles it, the noise added to the diagonal in fp64; lower triangle mirrored -> numpy [n, n]"""
    K = _ops.kernel_matrix(kind, X, None, var, ls).cpu().numpy()
    n = K.shape[0]
    K[np.arange(n), np.arange(n)] += noise
    M = np.tril(K) + np.tril(K, -1).T
    assert not np.isnan(M).any()
    return M


@pytest.mark.parametrize("kind,n,d,ard,dy", rr.resid_cases(), ids=["%s-%d-%d-%d" % (k, n, d, dy) for k, n, d, _, dy in rr.resid_cases()])
def test_residual_pass(device, kind, n, d, ard, dy):
    """gpn_refine_resid_part: Kyy a over the lower 64 x 64 tiles and their mirrors, Kyy re-computed from planted points, in
    double-double.  The whole tile range, and split into two calls whose hi + lo add up, against (1) the long-double Kyy a at the
    fp64-level tolerance of the kernel entries and (2) the assembled matrix times a in long double within n 2^-63 (|M| |a|)_i --
    which a plain fp64 product of the same matrix misses (asserted first)."""
    xn, ls, an = rr.resid_inputs(kind, n, d, ard, dy)
    noise = rr.RESID_NOISE
    X, var, lst, nz = _t(xn, device), _t([rr.VAR], device), _t(np.atleast_1d(ls), device), _t([noise], device)
    lds = _ops.round_up(n, _ops.LEAF)
    a = torch.zeros(dy, lds, dtype=torch.float64, device=device)
    a[:, :n] = _t(an, device)
    M = _assembled(kind, X, var, lst, noise)
    miss = rr.fp64_product_misses(M, an)
    assert min(miss) > 1.0, ("negative control", miss)
    ntile = (n + rr.RT - 1) // rr.RT
    ntri = ntile * (ntile + 1) // 2
    assert ntri == int(_native.lib().gpn_refine_tile_count(n))
    whole = _resid_part(kind, X, var, lst, nz, a, 0, ntri)
    cut = ntri // 2 + 1
    lo_, hi_ = _resid_part(kind, X, var, lst, nz, a, 0, cut), _resid_part(kind, X, var, lst, nz, a, cut, ntri)
    sums = {"whole": xr.ld(whole[..., 0]) + xr.ld(whole[..., 1]),
            "split": (xr.ld(lo_[..., 0]) + xr.ld(lo_[..., 1])) + (xr.ld(hi_[..., 0]) + xr.ld(hi_[..., 1]))}
    # (1) the long-double Kyy a
    Kyy = xr.K(kind, xn, None, rr.VAR, ls) + LD(noise) * np.eye(n, dtype=LD)
    want = xr.ld(an) @ Kyy
    e64 = xr.rel_err(xr.ld(an) @ xr.ld(rr.kyy64(kind, xn, ls, noise)), want)
    # (2) the assembled matrix
    exact, bound = rr.product_ld(M, an), rr.kyy_a_bound(M, an)
    keep = bound > 0
    pairs = []
    for what, got in sums.items():
        pairs.append(("Kyy_a " + what, xr.rel_err(got, want), xr.tol(e64, "K")))
        assert np.all(got[~keep] == 0)
        pairs.append(("assembled " + what, float(np.max(np.abs(got - exact)[keep] / bound[keep])), 1.0))
    report("resid", "%s-%d-%d-%d" % (kind, n, d, dy), pairs, "; fp64 control err/tol %.3g" % min(miss))


# ---------------------------------------------------------------------------------------------------------------------
# (c) the composed step at small sizes, recomputing and reading Kyy
# ---------------------------------------------------------------------------------------------------------------------
def _lml_check(out3, n, dy):
    """out3[2] against -1/2 out3[1] - dy out3[0] - 1/2 dy n log 2 pi in long double: (label, err, 4 roundings of the largest term)"""
    ref, big = rr.lml_term(out3[0], out3[1], n, dy)
    return ("LML term", abs(float(LD(out3[2]) - ref)), 4 * fr.U * big)


@pytest.mark.parametrize("kind,n,d,dy,ard,mean,noise", rr.STEP_CASES, ids=["%s-%d-%d-%d" % c[:4] for c in rr.STEP_CASES])
def test_refine_step_small(device, kind, n, d, dy, ard, mean, noise):
    """gpn_lml_refine below the sizes the shell applies it at, with and without a mean: the quadratic form pinned on the step's own
    intermediates (a_hat from gpn_backsub on the same factor, M the assembled Kyy, sum a_i (2 (y - m)_i - (M a)_i) in exact
    arithmetic), the LML term, the value against the long-double |alpha|^2; gpn_lml_refine_dense on the same matrix read from a
    buffer (ldk = n + 5, NaN in every tile above the diagonal tiles) gives the same three terms bit for bit."""
    lib = _native.lib()
    ident = "%s-%d-%d-%d" % (kind, n, d, dy)
    x, y, ls, mv = rr.step_inputs(kind, n, d, dy, ard, mean, noise)
    X, var, lst, nz = _t(x, device), _t([rr.VAR], device), _t(np.atleast_1d(ls), device), _t([noise], device)
    Y = _t(y, device)
    Mn = None if mv is None else _t(np.broadcast_to(mv, (n, dy)), device)
    R = Y if Mn is None else Y - Mn                                           # rounded once
    f, plain = _ops.lml_forward(kind, X, R, var, lst, nz, refine=False)
    assert f.jitter_rung == -1 and not f.refined
    plain = plain.cpu().numpy()
    work = _work(lib.gpn_lml_refine_work_bytes(n, dy), device)
    out = _t(plain, device)
    st = lib.gpn_lml_refine(_stream(device), _ops.KINDS[kind], _ptr(X), n, d, _ptr(Y), _ptr(Mn), dy, _ptr(var), _ptr(lst), lst.numel(), _ptr(nz),
                            _ptr(f.A), f.ld, _ptr(f.winv), _ptr(work), _ptr(out))
    _native.check(st, "gpn_lml_refine")
    out3 = out.cpu().numpy()
    assert out3[0] == plain[0] and not np.isnan(out3).any()
    # the step's own intermediates
    a_hat = _ops.backsub(f).cpu().numpy()
    M = _assembled(kind, X, var, lst, noise)
    quad = rr.step_quad_exact(R.cpu().numpy().T, M, a_hat)
    own_tol = 2 * fr.U * abs(float(quad)) + float(np.sum(np.abs(xr.ld(a_hat)) * rr.kyy_a_bound(M, a_hat)))
    pairs = [("own intermediates", rr.frac_err(out3[1], quad), own_tol), _lml_check(out3, n, dy)]
    # the truth
    ref = xr.GPRRef(x, y, kind, rr.VAR, ls, noise, ARD=ard, mean=mv)
    truth = np.sum(ref.alpha ** 2)
    dg = xr.DirectGPR(x, y, kind=kind, variance=rr.VAR, length_scales=ls, noise=noise, ARD=ard, mean=mv)
    with torch.no_grad():
        V = orc.trtrs(dg.Y - dg._mean(dg.X), orc.cholesky(dg.compute_kyy(dg.X)))
        e64 = xr.rel_err((V * V).sum().item(), truth)
    err_refined, err_plain = xr.rel_err(out3[1], truth), xr.rel_err(plain[1], truth)
    pairs.append(("|alpha|^2", err_refined, xr.tol(e64, "loss")))
    if noise < 1e-3:
        assert err_refined <= err_plain, (err_refined, err_plain)
    # the same step reading Kyy
    ldk = n + 5
    Kb = _full((n, ldk), NAN, device)
    Kb[:, :n] = _ops.kernel_matrix(kind, X, None, var, lst)
    tile = torch.arange(n, device=device) // rr.RT
    Kb[:, :n][tile[:, None] < tile[None, :]] = NAN
    work2 = _work(lib.gpn_lml_refine_work_bytes(n, dy), device)
    out2 = _t(plain, device)
    st = lib.gpn_lml_refine_dense(_stream(device), _ptr(Kb), ldk, float(noise), n, _ptr(Y), _ptr(Mn), dy, _ptr(f.A), f.ld, _ptr(f.winv),
                                  _ptr(work2), _ptr(out2))
    _native.check(st, "gpn_lml_refine_dense")
    assert np.array_equal(_bits(out2.cpu().numpy()), _bits(out3)), (out2.cpu().numpy(), out3)
    report("step", ident, pairs, "; own intermediates err/tol %.3g; |alpha|^2 rel. distance to long double: plain %.3g refined %.3g (e64 %.3g); "
           "dense: same bits" % (pairs[0][1] / pairs[0][2], err_plain, err_refined, e64))


# ---------------------------------------------------------------------------------------------------------------------
# (d) the finish
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dy,with_m", rr.FINISH_CASES, ids=["%d-%d-%s" % (n, dy, "m" if w else "nom") for n, dy, w in rr.FINISH_CASES])
def test_refine_finish(device, n, dy, with_m):
    """gpn_refine_finish on inputs that cancel (|quad| ~ 2^-22 sum |a_i t_i|) against exact rational arithmetic, at
    max(16 |finish_model - exact|, 2 u |quad|) -- which the plain fp64 sum of the same inputs misses by at least 100 x (asserted
    first; a single term, n dy = 1, cannot cancel: tests/test_refine_ref_host.py).  Either side of one element per thread of the one
    1024-thread workgroup; out3[0] is read and left alone."""
    y, m, a, ka_hi, ka_lo = rr.cancelling_finish_inputs(n, dy, seed=n + dy)
    if not with_m:
        y, m = y - m, None
    quad, S = rr.finish_exact(y, m, a, ka_hi, ka_lo)
    tol = rr.finish_tol(rr.finish_model(y, m, a, ka_hi, ka_lo), quad)
    miss = rr.frac_err(rr.finish_fp64(y, m, a, ka_hi, ka_lo), quad) / tol
    if n * dy > 1:
        assert abs(quad) <= S / 2 ** 20 and miss >= rr.FINISH_CONTROL_MISS, ("negative control", miss)
    lds = _ops.round_up(n, _ops.LEAF)
    ad, kad = _full((dy, lds), NAN, device), _full((dy, lds, 2), NAN, device)       # nothing past row n is read
    ad[:, :n] = _t(a, device)
    kad[:, :n, 0], kad[:, :n, 1] = _t(ka_hi, device), _t(ka_lo, device)
    logdet = 12.345 + n
    out = _t([logdet, NAN, NAN], device)
    Yd, Md = _t(y, device), (None if m is None else _t(m, device))
    st = _native.lib().gpn_refine_finish(_stream(device), _ptr(Yd), _ptr(Md), _ptr(ad), _ptr(kad), n, dy, _ptr(out))
    _native.check(st, "gpn_refine_finish")
    out3 = out.cpu().numpy()
    assert out3[0] == logdet
    err = rr.frac_err(out3[1], quad)
    report("finish", "%d-%d-%s" % (n, dy, "m" if with_m else "nom"), [("quad", err, tol), _lml_check(out3, n, dy)],
           "; quad err/tol %.3g, |quad|/S 2^%.1f, fp64 control err/tol %.3g" % (err / tol, np.log2(float(abs(quad) / S)), miss))


# ---------------------------------------------------------------------------------------------------------------------
# (e) gemv_t
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dy", rr.GEMV_DY)
@pytest.mark.parametrize("rows,cols", rr.GEMV_SHAPES)
def test_gemv_t_acc(device, rows, cols, dy):
    """gpn_gemv_t_acc: c += L^T a against long double, relative to |c0| + |L|^T |a| per column; around 32 rows per chunk and 256
    columns per workgroup; padding of L and a is NaN (not read), columns >= cols of c keep their sentinel; a scratch sized for the
    widest shape of the table gives the same bits (gpn_gemv_t_work_bytes is monotone in the width: tests/test_abi.py)."""
    lib = _native.lib()
    L, a, c0 = rr.gemv_inputs(rows, cols, dy)
    ld, lda, ldc = cols + 3, rows + 2, cols + 3
    Ld, ad = _full((rows, ld), NAN, device), _full((dy, lda), NAN, device)
    Ld[:, :cols], ad[:, :rows] = _t(L, device), _t(a, device)
    wide = max(c for _, c in rr.GEMV_SHAPES)
    assert lib.gpn_gemv_t_work_bytes(rows, wide, dy) >= lib.gpn_gemv_t_work_bytes(rows, cols, dy)
    runs = []
    for nbytes in (lib.gpn_gemv_t_work_bytes(rows, cols, dy), lib.gpn_gemv_t_work_bytes(rows, wide, dy)):
        cd = _full((dy, ldc), SENTINEL, device)
        cd[:, :cols] = _t(c0, device)
        work = _work(nbytes, device)
        st = lib.gpn_gemv_t_acc(_stream(device), _ptr(Ld), ld, rows, cols, _ptr(ad), lda, dy, _ptr(cd), ldc, _ptr(work))
        _native.check(st, "gpn_gemv_t_acc")
        c = cd.cpu().numpy()
        assert np.all(c[:, cols:] == SENTINEL) and not np.isnan(c).any()
        runs.append(c[:, :cols].copy())
    assert np.array_equal(_bits(runs[0]), _bits(runs[1]))
    e64 = rr.gemv_metric(c0 + a @ L, L, a, c0)
    report("gemv_t", "%d-%d-%d" % (rows, cols, dy), [("c0 + L^T a", rr.gemv_metric(runs[0], L, a, c0), fr.tol(e64))])
