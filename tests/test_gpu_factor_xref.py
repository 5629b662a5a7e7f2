"""The dense linear algebra under every model -- gpn_potrf_lower and its drivers (potrf.hip, leaf16*.h, colpanel.hip, ppotrf.hip) and
the triangular kernels (trisolve.hip) -- against the long-double reference of tests/_xref.py, on the matrix families, metrics
and tolerance rule of tests/_factor_ref.py:  tol = max(16 e64, 8 * 2^-53), e64 = the larger error of an fp64 model of the kernels'
algorithm and of LAPACK in the same metric, computed here on the CPU.  Every test prints its worst err / tol ("XREF ..." lines).

The factorisation goes through _ops.Factor with gpn_copy_matrix, pack_rhs and potrf() called directly: no jitter ladder."""
import contextlib

import numpy as np
import pytest
import torch

from gptorch_amd import _native, _ops, functions, rng
from gptorch_amd._ops import _ptr, _stream
from tests import _factor_ref as fr
from tests import _xref as xr

pytestmark = pytest.mark.gpu

LEAF = fr.LEAF
# id -> (gpn_debug_set_potrf_variant, gpn_debug_set_outer_width): parametrisations of the shipped driver (potrf.hip)
DRIVERS = {
    "A": (1, 0, 0),             # plain recursion
    "B": None,                  # the shipped library and its defaults: 256-wide panels, one level below 2048
    "C": (0x100, 256, 512),     # three levels 128:256:512 -- the trapezoid (lower = 2) updates
    "D": (0x420, -1, 0),        # one level of 512, right-looking aux-stream fork
    "E": (0x408, -1, 0),        # the same, left-looking
    "F": (0x300, 0, 0),         # 384-wide panels
}
SIZES = [(1, 0), (2, 1), (127, 3), (128, 0), (129, 1), (256, 3), (257, 0), (385, 17), (641, 3), (1100, 9)]
ALL_FAMILIES_AT = [(129, 1), (385, 17), (641, 3), (1100, 9)]
TRI_FAMILIES = ("well", "graded10", "rbf_ill")


@contextlib.contextmanager
def driver(name):
    if DRIVERS[name] is None:
        yield
        return
    v, w1, w2 = DRIVERS[name]
    dbg = _native.debug_begin()
    dbg.gpn_debug_set_potrf_variant(v)
    dbg.gpn_debug_set_outer_width(w1, w2)
    try:
        yield
    finally:
        dbg.gpn_debug_set_potrf_variant(0)
        dbg.gpn_debug_set_outer_width(0, 0)
        _native.debug_end()


def _t(a, device):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=device)


def load(f, A, R=None, tril=1):
    """matrix (and right-hand sides R [n, e]) into the factor buffer: gpn_copy_matrix + gpn_pack_rhs"""
    n = f.n
    src = _t(A, f.device)
    _native.check(_native.lib().gpn_copy_matrix(_stream(f.device), _ptr(src), n, n, n, _ptr(f.A), f.ld, tril), "gpn_copy_matrix")
    if f.e:
        f.pack_rhs(_t(R, f.device))


def result(f):
    """(L, extra rows, leaf inverses [blocks, 128, 128], lml terms) as numpy"""
    return (f.lower().cpu().numpy(), f.extra().cpu().numpy().copy(), f.winv.cpu().numpy().reshape(-1, LEAF, LEAF).copy(),
            f.lml_terms().cpu().numpy())


def factorise(name, A, R, device, f=None, tril=1):
    n, e = A.shape[0], (0 if R is None else R.shape[1])
    f = _ops.Factor(n, e, device) if f is None else f
    with driver(name):
        load(f, A, R, tril)
        info = f.potrf()
        out = result(f)
    return info, out, f


def report(what, ident, pairs):
    """pairs: (label, err, tol) -> prints the worst err / tol and asserts every one"""
    worst = max(pairs, key=lambda p: p[1] / p[2])
    print("XREF %s %s worst %s err/tol %.3f (err %.3g = %.1f u)" % (what, ident, worst[0], worst[1] / worst[2], worst[1], worst[1] / fr.U))
    for label, err, t in pairs:
        assert err <= t, (what, ident, label, "err %.3g tol %.3g (%.1f u)" % (err, t, err / fr.U))


def winv_structure_ok(W, n):
    """exactly zero above the diagonal of every leaf inverse and outside the kb x kb corner of a ragged last leaf"""
    for b, k in enumerate(range(0, n, LEAF)):
        kb = min(LEAF, n - k)
        keep = np.tril(np.ones((LEAF, LEAF), dtype=bool))
        keep[kb:, :] = False
        keep[:, kb:] = False
        if W[b][~keep].any():
            return False
    return True


@pytest.fixture(scope="module")
def refs():
    """long-double reference + e64 of (family, n, e): computed once per module"""
    cache = {}

    def get(family, n, e):
        if (family, n) not in cache:
            A = fr.matrix(family, n)
            cache[family, n] = fr.FactorRef(A, fr.rhs(A, e) if e else None)
        return cache[family, n]
    return get


def _factor_cases():
    out = []
    for drv in "ABCDEF":
        for n, e in (SIZES if drv in "AB" else [(641, 3), (1100, 9)]):
            for fam in (fr.FAMILIES if (n, e) in ALL_FAMILIES_AT else ("well",)):
                out.append(pytest.param(drv, n, e, fam, id="%s-%d-%d-%s" % (drv, n, e, fam)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 2. the factorisation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drv,n,e,family", _factor_cases())
def test_factor_against_long_double(device, refs, drv, n, e, family):
    """factor, leaf inverses, extra rows and the three LML terms of every driver parametrisation, at the leaf / panel edges and on
    graded and ill-conditioned matrices."""
    ref = refs(family, n, e)
    info, (L, E, W, T), _ = factorise(drv, ref.A, ref.R, device)
    assert info == 0
    assert np.array_equal(np.triu(L, 1), np.zeros_like(L))
    ident = "%s-%d-%d-%s" % (drv, n, e, family)
    pairs = [("forward", ref.forward(L), fr.tol(ref.e64["forward"])), ("residual", ref.residual(L), fr.tol(ref.e64["residual"]))]
    report("factor", ident, pairs)
    assert winv_structure_ok(W, n)
    report("leaf", ident, [("block %d" % k, err, fr.tol(e64)) for k, (err, e64) in enumerate(zip(ref.leaf_errs(W), ref.e64["leaf"]))])
    if e:
        report("extra", ident, [("extra rows", ref.extra_err(E), fr.tol(ref.e64["extra"]))])
    names = ("sum log L_ii", "sum of squares", "LML")
    report("lml", ident, [(names[i], abs(float(xr.LD(T[i]) - ref.lml_ref[i])), ref.lml_tol()[i]) for i in range(3 if e else 1)])


@pytest.mark.parametrize("drv", ["B", "C"])
@pytest.mark.parametrize("n,e", [(641, 3), (1100, 9)])
def test_power_of_two_scaling_is_exact(device, refs, drv, n, e):
    """graded2 = D well D with D = diag(2^k): every operation of the kernels (fma, rsq of 4^k d and its refinement, MFMA) scales
    exactly while nothing leaves the normal range, so the factor is D times well's factor and the leaf inverses are well's times
    D^-1 BIT FOR BIT; the extra rows (L^-1 R with R scaled by D as well) are the SAME bits.  sum log L_ii is not exact: log(2^k l)
    is rounded once more than log(l) + k log 2 -- the one legitimate approximation here, so sum log L_ii - sum k_i log 2 is held to
    the tolerance rule of the LML terms instead."""
    r0, r2 = refs("well", n, e), refs("graded2", n, e)
    k = fr.graded2_exponents(n)
    d = np.ldexp(1.0, k)
    assert np.array_equal(r2.A, r0.A * d[:, None] * d[None, :]) and np.array_equal(r2.R, r0.R * d[:, None])
    i0, (L0, E0, W0, T0), _ = factorise(drv, r0.A, r0.R, device)
    i2, (L2, E2, W2, T2), _ = factorise(drv, r2.A, r2.R, device)
    assert i0 == 0 and i2 == 0
    bad = np.argwhere(L2 != L0 * d[:, None])
    assert bad.size == 0, ("factor", len(bad), bad[:5].tolist())
    bad = np.argwhere(E2 != E0)
    assert bad.size == 0, ("extra rows", len(bad), bad[:5].tolist())
    for b, c0 in enumerate(range(0, n, LEAF)):
        kb = min(LEAF, n - c0)
        bad = np.argwhere(W2[b, :kb, :kb] != W0[b, :kb, :kb] / d[None, c0:c0 + kb])
        assert bad.size == 0, ("leaf inverse", b, len(bad), bad[:5].tolist())
    shift = float(np.sum(xr.ld(k)) * np.log(xr.LD(2)))
    err = abs(float(xr.LD(T2[0]) - xr.LD(shift) - xr.LD(T0[0])))
    t = r0.lml_tol()[0] + r2.lml_tol()[0]
    print("XREF scaling %s-%d bitwise factor / extra rows / leaf inverses; sum log err/tol %.3f" % (drv, n, err / t))
    assert err <= t


@pytest.mark.parametrize("drv", ["B", "C"])
@pytest.mark.parametrize("n,e", [(641, 3), (1100, 9)])
def test_strict_upper_triangle_is_not_read(device, refs, drv, n, e):
    """gpnative.h: the strict upper triangle of the n x n block is not read (and unspecified on exit): with A[i, j > i] = NaN on
    entry the lower triangle of L, the extra rows, the leaf inverses and info are the bits of the clean run."""
    ref = refs("well", n, e)
    i0, (L0, E0, W0, T0), _ = factorise(drv, ref.A, ref.R, device)
    An = np.tril(ref.A) + np.triu(np.full((n, n), np.nan), 1)
    i1, (L1, E1, W1, T1), _ = factorise(drv, An, ref.R, device, tril=0)
    assert i0 == 0 and i1 == 0
    assert np.array_equal(L1, L0) and np.array_equal(E1, E0) and np.array_equal(W1, W0) and np.array_equal(T1, T0)


# ---------------------------------------------------------------------------------------------------------------------
# 3. exact info
# ---------------------------------------------------------------------------------------------------------------------
_clean = {}


def _clean_bits(drv, device):
    if drv not in _clean:
        A = fr.well(fr.INFO_N)
        info, out, _ = factorise(drv, A, fr.rhs(A, 3), device)
        assert info == 0
        _clean[drv] = (A, fr.rhs(A, 3), out)
    return _clean[drv]


@pytest.mark.parametrize("pivots,nans", fr.planted_cases(), ids=fr.planted_ids())
@pytest.mark.parametrize("drv", ["A", "B", "C", "D"])
def test_info_is_the_first_failing_pivot(device, drv, pivots, nans):
    """gpnative.h: info = j > 0: the leading minor of order j is not positive definite (first failing pivot, 1-based).  `well` has
    pivots >= 0.5, so P[j-1, j-1] = -1 fails at exactly j; of two failures the lower index wins; a NaN at A[i, c] (c < i) fails
    row i's pivot.  A clean matrix factored into the same buffers afterwards gives info 0 and the clean bits."""
    A, R, (L0, E0, W0, T0) = _clean_bits(drv, device)
    P, expect = fr.planted(fr.INFO_N, pivots, nans)
    info, _, f = factorise(drv, P, R, device)
    assert info == expect
    info, (L1, E1, W1, T1), _ = factorise(drv, A, R, device, f=f)
    assert info == 0
    assert np.array_equal(L1, L0) and np.array_equal(E1, E0) and np.array_equal(W1, W0) and np.array_equal(T1, T0)


def test_info_of_the_lock_step_factorisation(device):
    """gpn_potrf_lower_batched: every problem its own info; the clean problems are bit-identical to their sequential factors"""
    n, e, B = 385, 1, 4
    mats = [fr.planted(n, (17,), seed=0)[0], fr.well(n, 1), fr.planted(n, (257,), seed=2)[0], fr.well(n, 3)]
    Rs = [fr.rhs(fr.well(n, s), e, seed=s) for s in range(B)]
    fb = _ops.FactorBatch(B, n, e, device)
    for b in range(B):
        load(fb.factor(b), mats[b], Rs[b])
    fb.info.zero_()
    st = _native.lib().gpn_potrf_lower_batched(_stream(device), _ptr(fb.A), n, e, fb.ld, fb.sA, _ptr(fb.winv), fb.sW, _ptr(fb.info), B)
    assert st == 0
    assert fb.info.tolist() == [17, 0, 257, 0]
    for b in (1, 3):
        info, (L0, E0, W0, T0), _ = factorise("B", mats[b], Rs[b], device)
        assert info == 0
        L1, E1, W1, T1 = result(fb.factor(b))
        assert np.array_equal(L1, L0) and np.array_equal(E1, E0) and np.array_equal(W1, W0) and np.array_equal(T1, T0)


def test_info_of_the_persistent_factorisation(device):
    """gpn_potrf_lower_persistent at its smallest size: the index of gpn_potrf_lower, and equal to the planted pivot"""
    n, e = 2560, 1
    lib = _native.lib()
    assert lib.gpn_potrf_persistent_supported(n, e) == 1
    R = fr.rhs(fr.well(n), e)
    f = _ops.Factor(n, e, device)
    for j in (129, n):
        P, expect = fr.planted(n, (j,))
        got = []
        for fn in (lib.gpn_potrf_lower, lib.gpn_potrf_lower_persistent):
            load(f, P, R)
            f.info.zero_()
            assert fn(_stream(device), _ptr(f.A), n, e, f.ld, _ptr(f.winv), _ptr(f.info)) == 0
            got.append(int(f.info.item()))
        assert got == [expect, expect] and expect == j


# ---------------------------------------------------------------------------------------------------------------------
# 4. triangular kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gfactors(device):
    """the shipped driver's factor of (family, n): (Factor, A, L as fp64 numpy, sqrt(a_ii))"""
    cache = {}

    def get(family, n):
        if (family, n) not in cache:
            A = fr.matrix(family, n)
            info, out, f = factorise("B", A, None, device)
            assert info == 0
            cache[family, n] = (f, A, out[0], np.sqrt(np.diag(A)))
        return cache[family, n]
    return get


def _rhs_buffer(f, Rt):
    """[m, n] right-hand sides in a zero-padded buffer shaped like the factor's"""
    m = Rt.shape[0]
    B = _ops.padded_like_factor(f, m)
    B[:m, :f.n] = _t(Rt, f.device)
    return B


@pytest.mark.parametrize("n", [129, 385, 1100])
@pytest.mark.parametrize("m", [1, 17, 130])
def test_trsm_right_lt(device, gfactors, n, m):
    """gpn_trsm_right_lt: X L^T = B against long-double substitution with the SAME (native) L; gpn_trsm_right_lt_batched over the
    three families' factors is bit-identical per problem."""
    lib = _native.lib()
    single, pairs = [], []
    for fam in TRI_FAMILIES:
        f, A, L, sd = gfactors(fam, n)
        R = fr.rhs(A, m, seed=m)
        B = _rhs_buffer(f, R.T)
        f.solve_right_lt(B, m)
        X = B[:m, :n].cpu().numpy()
        ref = xr.solve_lower(xr.ld(L), R)
        pairs.append((fam, xr.abs_err(X.T, ref), fr.tol(fr.solve_e64(L, R, ref))))
        single.append((R, X))
    report("trsm", "%d-%d" % (n, m), pairs)
    fb = _ops.FactorBatch(3, n, 0, device)
    rows = _ops.round_up(m, LEAF)
    Bb = _ops.zeros(3 * rows, fb.ld, device)
    for b, fam in enumerate(TRI_FAMILIES):
        f = gfactors(fam, n)[0]
        fb.A[b * fb.rows:(b + 1) * fb.rows].copy_(f.A)
        fb.winv[b * fb.sW:b * fb.sW + f.winv.numel()].copy_(f.winv)
        Bb[b * rows:b * rows + m, :n] = _t(single[b][0].T, device)
    st = lib.gpn_trsm_right_lt_batched(_stream(device), _ptr(fb.A), n, fb.ld, fb.sA, _ptr(fb.winv), fb.sW, _ptr(Bb), m, fb.ld, rows * fb.ld, 3)
    assert st == 0
    for b in range(3):
        assert np.array_equal(Bb[b * rows:b * rows + m, :n].cpu().numpy(), single[b][1]), TRI_FAMILIES[b]


@pytest.mark.parametrize("n", [129, 385, 1100])
@pytest.mark.parametrize("family", TRI_FAMILIES)
def test_trtri_upper(device, gfactors, family, n):
    """U = L^-T by gpn_trtri_upper, gpn_trtri_upper_ws and gpn_trtri_upper_batched against the long-double inverse of the native L
    (entries weighed by sqrt(a_ii): row i of U scales like 1 / sqrt(a_ii)); strict lower triangle exactly zero; the batched form is
    bit-identical to gpn_trtri_upper up to n = 256 and to gpn_trtri_upper_ws above (gpnative.h)."""
    lib = _native.lib()
    s = _stream(device)
    f, A, L, sd = gfactors(family, n)
    Wref = fr.lower_inverse_ld(xr.ld(L))
    eye = np.eye(n)
    e64 = max(float(np.max(np.abs(xr.ld(fr.model_solve(L, eye)) - Wref) * sd[None, :])),
              float(np.max(np.abs(xr.ld(torch.linalg.solve_triangular(torch.tensor(L), torch.eye(n, dtype=torch.float64), upper=False).numpy())
                                  - Wref) * sd[None, :])))
    fs = [gfactors(fam, n)[0] for fam in TRI_FAMILIES]
    mine = TRI_FAMILIES.index(family)
    U0s, U1s = [], []
    for g in fs:
        U0 = _ops.zeros(g.rows, g.ld, device)
        assert lib.gpn_trtri_upper(s, _ptr(g.A), n, g.ld, _ptr(g.winv), _ptr(U0), g.ld) == 0
        U1, S1 = _ops.zeros(g.rows, g.ld, device), _ops.zeros(g.rows, g.ld, device)
        assert lib.gpn_trtri_upper_ws(s, _ptr(g.A), n, g.ld, _ptr(g.winv), _ptr(U1), g.ld, _ptr(S1), g.ld) == 0
        U0s.append(U0[:n, :n].cpu().numpy())
        U1s.append(U1[:n, :n].cpu().numpy())
    fb = _ops.FactorBatch(3, n, 0, device)
    for b, g in enumerate(fs):
        fb.A[b * fb.rows:(b + 1) * fb.rows].copy_(g.A)
        fb.winv[b * fb.sW:b * fb.sW + g.winv.numel()].copy_(g.winv)
    Ub, Sb = _ops.zeros(3 * fb.rows, fb.ld, device), _ops.zeros(3 * fb.rows, fb.ld, device)
    st = lib.gpn_trtri_upper_batched(s, _ptr(fb.A), n, fb.ld, fb.sA, _ptr(fb.winv), fb.sW, _ptr(Ub), fb.ld, fb.sA, _ptr(Sb), fb.ld, fb.sA, 3)
    assert st == 0
    U2s = [Ub[b * fb.rows:b * fb.rows + n, :n].cpu().numpy() for b in range(3)]
    for b in range(3):
        assert np.array_equal(U2s[b], U0s[b] if n <= 2 * LEAF else U1s[b]), TRI_FAMILIES[b]
    pairs = []
    for name, U in (("trtri_upper", U0s[mine]), ("trtri_upper_ws", U1s[mine]), ("trtri_upper_batched", U2s[mine])):
        assert np.array_equal(np.tril(U, -1), np.zeros_like(U)), name
        pairs.append((name, float(np.max(np.abs(xr.ld(U).T - Wref) * sd[None, :])), fr.tol(e64)))
    report("trtri", "%s-%d" % (family, n), pairs)


@pytest.mark.parametrize("n", [1025, 1153])
@pytest.mark.parametrize("family", TRI_FAMILIES)
def test_block_inverse_and_blocked_solve(device, gfactors, family, n):
    """gpn_block_inverse: two 1024-blocks, the last one ragged (1 and 129 columns), against the long-double L_bb^-1 of the native
    L, zero above the diagonal and beyond the ragged edge; gpn_trsm_right_lt_blocked with 1 and 37 right-hand sides against
    long-double substitution (e64: the fp64 model with explicit inverses of the 1024-blocks, or LAPACK)."""
    lib = _native.lib()
    BIG = 1024
    f, A, L, sd = gfactors(family, n)
    nb = (n + BIG - 1) // BIG
    wb = _ops.block_inverses(f)
    blocks = wb[:nb * BIG * BIG].view(nb, BIG, BIG).cpu().numpy()
    pairs = []
    for b in range(nb):
        c0, c1 = b * BIG, min(n, (b + 1) * BIG)
        k = c1 - c0
        keep = np.tril(np.ones((BIG, BIG), dtype=bool))
        keep[k:, :] = False
        keep[:, k:] = False
        assert not blocks[b][~keep].any(), b
        Lb = np.ascontiguousarray(L[c0:c1, c0:c1])
        Wref = fr.lower_inverse_ld(xr.ld(Lb))
        s = sd[None, c0:c1]
        lap = torch.linalg.solve_triangular(torch.tensor(Lb), torch.eye(k, dtype=torch.float64), upper=False).numpy()
        e64 = max(float(np.max(np.abs(xr.ld(fr.model_solve(Lb, np.eye(k))) - Wref) * s)), float(np.max(np.abs(xr.ld(lap) - Wref) * s)))
        pairs.append(("block %d" % b, float(np.max(np.abs(xr.ld(blocks[b][:k, :k]) - Wref) * s)), fr.tol(e64)))
    report("block_inverse", "%s-%d" % (family, n), pairs)
    pairs = []
    for m in (1, 37):
        R = fr.rhs(A, m, seed=m)
        B, X = _rhs_buffer(f, R.T), _ops.padded_like_factor(f, m)
        st = lib.gpn_trsm_right_lt_blocked(_stream(device), _ptr(f.A), n, f.ld, _ptr(wb), _ptr(B), m, B.stride(0), _ptr(X), X.stride(0))
        assert st == 0
        ref = xr.solve_lower(xr.ld(L), R)
        pairs.append(("m = %d" % m, xr.abs_err(X[:m, :n].cpu().numpy().T, ref), fr.tol(fr.solve_e64(L, R, ref, nb=BIG))))
    report("trsm_blocked", "%s-%d" % (family, n), pairs)


@pytest.mark.parametrize("n", [1, 127, 129, 300])
def test_general_triangular_matrix(device, n):
    """gpn_trtri_diag and functions.trtrs with a triangular matrix that is NOT a Cholesky factor (diagonal of mixed sign): the leaf
    inverses, functions.trtrs(b, T) and functions.trtrs(b, T^T, lower=False) against long-double substitution; e64 from
    torch.linalg.solve_triangular on the CPU."""
    T = fr.triangular(n)
    b = rng.normal(7800 + n, (n, 3))
    Tl = xr.ld(T)
    Tt, bt = _t(T, device), _t(b, device)
    f = _ops.Factor(n, 0, device)
    lib = _native.lib()
    _native.check(lib.gpn_copy_matrix(_stream(device), _ptr(Tt), n, n, n, _ptr(f.A), f.ld, 1), "gpn_copy_matrix")
    assert lib.gpn_trtri_diag(_stream(device), _ptr(f.A), n, f.ld, _ptr(f.winv), _ptr(f.info)) == 0
    assert int(f.info.item()) == 0
    W = f.winv.cpu().numpy().reshape(-1, LEAF, LEAF)
    assert winv_structure_ok(W, n)
    pairs = []
    for k, c0 in enumerate(range(0, n, LEAF)):
        c1 = min(n, c0 + LEAF)
        Tb = np.ascontiguousarray(T[c0:c1, c0:c1])
        eye = np.eye(c1 - c0, dtype=xr.LD)
        lap = torch.linalg.solve_triangular(torch.tensor(Tb), torch.eye(c1 - c0, dtype=torch.float64), upper=False).numpy()
        e64 = float(np.max(np.abs(np.einsum("ik,kj->ij", xr.ld(lap), xr.ld(Tb)) - eye)))
        err = float(np.max(np.abs(np.einsum("ik,kj->ij", xr.ld(W[k, :c1 - c0, :c1 - c0]), xr.ld(Tb)) - eye)))
        pairs.append(("leaf %d" % k, err, fr.tol(e64)))
    x = functions.trtrs(bt, Tt).cpu().numpy()
    ref = xr.solve_lower(Tl, b)
    lap = torch.linalg.solve_triangular(torch.tensor(T), torch.tensor(b), upper=False).numpy()
    pairs.append(("trtrs lower", xr.abs_err(x, ref), fr.tol(xr.abs_err(lap, ref))))
    xu = functions.trtrs(bt, Tt.t(), lower=False).cpu().numpy()
    refu = xr.solve_upper_t(Tl, b)
    lapu = torch.linalg.solve_triangular(torch.tensor(T).t(), torch.tensor(b), upper=True).numpy()
    pairs.append(("trtrs upper", xr.abs_err(xu, refu), fr.tol(xr.abs_err(lapu, refu))))
    report("general_triangular", str(n), pairs)


@pytest.mark.parametrize("j", [1, 128, 129, 300])
def test_zero_pivot_of_a_triangular_matrix(device, j):
    """gpnative.h: gpn_trtri_diag's info = j > 0: zero pivot at column j; functions.trtrs raises naming it"""
    n = 300
    T = fr.triangular(n)
    T[j - 1, j - 1] = 0.0
    Tt = _t(T, device)
    f = _ops.Factor(n, 0, device)
    lib = _native.lib()
    _native.check(lib.gpn_copy_matrix(_stream(device), _ptr(Tt), n, n, n, _ptr(f.A), f.ld, 1), "gpn_copy_matrix")
    assert lib.gpn_trtri_diag(_stream(device), _ptr(f.A), n, f.ld, _ptr(f.winv), _ptr(f.info)) == 0
    assert int(f.info.item()) == j
    with pytest.raises(RuntimeError, match=r"zero pivot %d\)" % j):
        functions.trtrs(_t(rng.normal(3, (n, 2)), device), Tt)


def test_potrf_lower_panel_stays_left_of_column_n(device):
    """gpn_potrf_lower_panel, a tile column of a larger matrix: n = 384, 300 panel rows below, buffer ld = 512 whose columns
    384 .. 511 hold NaN in every row of the tile column: the panel rows come out as R L^-T, info = 0 and the NaN columns keep their
    bits (nothing right of column n is read or written)."""
    n, e, ld = 384, 300, 512
    full = fr.well(n + e)
    A, R = full[:n, :n], np.ascontiguousarray(full[n:, :n].T)          # R [n, e]: the panel rows are R^T
    ref = fr.FactorRef(A, R)
    rows = _ops.round_up(n + e, LEAF) + 16
    buf = _ops.zeros(rows, ld, device)
    buf[:n + e, :n] = _t(np.vstack([np.tril(A), R.T]), device)
    buf[:n + e, n:] = float("nan")
    before = buf[:, n:].clone()
    winv = torch.empty(3 * LEAF * LEAF, dtype=torch.float64, device=device)
    info = torch.zeros(1, dtype=torch.int32, device=device)
    st = _native.lib().gpn_potrf_lower_panel(_stream(device), _ptr(buf), n, e, ld, _ptr(winv), _ptr(info))
    assert st == 0 and int(info.item()) == 0
    assert torch.equal(buf[:, n:].view(torch.int64), before.view(torch.int64))
    L = torch.tril(buf[:n, :n]).cpu().numpy()
    W = winv.cpu().numpy().reshape(-1, LEAF, LEAF)
    assert winv_structure_ok(W, n)
    report("panel", "384-300", [("forward", ref.forward(L), fr.tol(ref.e64["forward"])),
                                ("residual", ref.residual(L), fr.tol(ref.e64["residual"])),
                                ("panel rows", ref.extra_err(buf[n:n + e, :n].cpu().numpy()), fr.tol(ref.e64["extra"]))]
           + [("leaf %d" % k, err, fr.tol(e64)) for k, (err, e64) in enumerate(zip(ref.leaf_errs(W), ref.e64["leaf"]))])
