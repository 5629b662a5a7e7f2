"""The fp64 MFMA contraction (csrc/gemm_f64.hip, csrc/gemm_tile.h) against the long-double reference of tests/_gemm_ref.py on
full-mantissa data: every comparison entrywise within bound(K, S) = (K + 3) 2^-53 S (derived from the operation count, see
_gemm_ref.py), and bit for bit wherever the ABI or the lock-step drivers promise identical results -- across tile shapes, strides,
padding contents, the thin-tile path, the K clipping of triangular operands and the batched entry points.  tests/test_gpu_gemm.py
keeps the exact-integer checks of the fragment maps and tile walks; this module sees what integers cannot."""
import contextlib

import numpy as np
import pytest
import torch

from gptorch_amd import _native, _ops
from tests import _gemm_ref as gr

pytestmark = pytest.mark.gpu

LD = gr.LD
F64 = torch.float64
UU = gr.TRI_A_UPPER | gr.TRI_B_UPPER
PIPELINED = (7, 8, 9, 11)              # the tile shapes that have the thin-tile path (the software-pipelined K loop)


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def forced(variant, thin=None):
    """the tools' build with one tile shape (and, optionally, the thin-tile switch) for this thread's launches"""
    lib = _native.debug_begin()
    try:
        lib.gpn_debug_set_gemm_variant(variant)
        if thin is not None:
            lib.gpn_debug_set_thin_tiles(thin)
        yield lib
    finally:
        lib.gpn_debug_set_thin_tiles(1)
        _native.debug_end()


def rows16(X, device, fill=0.0):
    """X on the device with its rows padded to a multiple of 16 by `fill` (the ABI only asks for those rows to be readable)"""
    t = torch.full((gr.round_up(X.shape[0], 16), X.shape[1]), fill, dtype=F64, device=device)
    t[:X.shape[0]] = dev(X, device)
    return t


def dev(X, device):
    return torch.from_numpy(np.array(X, order="C")).to(device)      # a copy: the shared cases are read-only


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def all_bits(t, value):
    return same_bits(t, torch.full_like(t, value))


def inside(C, ref, S, K, tiny=0.0, mask=None, c0=None):
    """|C - ref| <= bound(K, S, tiny) on every entry (a NaN fails); entries outside `mask` must hold the bits of c0.
    -> worst err / unit of the bound"""
    got = C.detach().cpu().numpy()
    err = np.abs(gr.ld(got) - ref)
    lim = gr.bound(K, S, tiny)
    if mask is not None:
        assert np.array_equal(got[~mask].view(np.int64), np.ascontiguousarray(c0)[~mask].view(np.int64)), "wrote outside the mask"
        err, lim = err[mask], lim[mask]
    bad = ~(err <= lim)
    assert not bad.any(), "%d entries outside the bound, worst err / bound %.3g" % (
        int(bad.sum()), float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1), np.where(err > 0, np.inf, 0)))))
    return gr.units(got, ref, S, K, tiny)


def gemm(Ad, Bd, M, N, K, alpha, beta, C0d, lower=0, tri=0):
    C = C0d.clone()
    _ops.gemm_nt(Ad, Bd, M, N, K, alpha=alpha, beta=beta, C=C, lower=lower, tri=tri)
    return C


def numpy_units(A, B, C0, alpha, beta, ref, S, K, tiny):
    got = alpha * (A @ B.T) + (beta * C0 if beta != 0.0 else 0.0)
    return gr.units(got, ref, S, K, tiny)


# ---------------------------------------------------------------------------------------------------------------------
# 1. accuracy, full rectangle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", gr.FAMILIES)
@pytest.mark.parametrize("variant", gr.VARIANTS)
def test_accuracy_full_rectangle(device, variant, family):
    """every shape x tile shape x family, the (alpha, beta) pairs dealt over the cases: |C - ref| <= (K + 3) 2^-53 S entry by
    entry (`tiny`: + K 2^-1074 -- the MI355X keeps subnormal MFMA products and sums, LAB.md section 28).  The `tri` family runs
    with its flags (A_UPPER | B_UPPER)."""
    worst = worst_np = 0.0
    with forced(variant):
        for si, (M, N, K) in enumerate(gr.SHAPES):
            A, B, C0, P, SP = gr.case(family, M, N, K)
            alpha, beta = gr.pair_of(si, gr.VARIANTS.index(variant), gr.FAMILIES.index(family))
            tiny = gr.tiny_of(family, K)
            ref, S = gr.combine(P, SP, C0, alpha, beta)
            C = gemm(rows16(A, device), rows16(B, device), M, N, K, alpha, beta, dev(C0, device), tri=UU if family == "tri" else 0)
            worst = max(worst, inside(C, ref, S, K, tiny))
            worst_np = max(worst_np, numpy_units(A, B, C0, alpha, beta, ref, S, K, tiny))
    print("gemm xref: variant %2d %-6s worst err / (2^-53 S) = %5.2f   (numpy fp64: %5.2f)" % (variant, family, worst, worst_np))


# ---------------------------------------------------------------------------------------------------------------------
# 2. lower = 1, lower = 2, staircase
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", gr.VARIANTS)
def test_lower_and_trapezoid(device, variant):
    """lower = 1 (n in 1, 33, 130, 257; K in 16, 80) and lower = 2 ((130, 64), (300, 129), (257, 257)): the same bound on the
    entries with j <= i, the sentinel's bits everywhere else"""
    cases = [(n, n, K, 1) for n, K in gr.LOWER1] + [(M, N, K, 2) for M, N, K in gr.LOWER2]
    with forced(variant):
        for ci, (M, N, K, lower) in enumerate(cases):
            for fi, family in enumerate(("scaled", "cancel", "tiny")):
                A, B, C0, P, SP = gr.case(family, M, N, K)
                alpha, beta = gr.pair_of(ci, fi, variant)
                mask = gr.mask_lower(M, N)
                c0 = np.where(mask, C0, gr.SENTINEL)
                ref, S = gr.combine(P, SP, c0, alpha, beta, mask)
                C = gemm(rows16(A, device), rows16(B, device), M, N, K, alpha, beta, dev(c0, device), lower=lower)
                inside(C, ref, S, K, gr.tiny_of(family, K), mask, c0)


@pytest.mark.parametrize("variant", gr.VARIANTS)
def test_staircase(device, variant):
    """gpn_gemm_nt_stair with 128-column blocks on every tile shape (all are square): (300, 2, 128, 1), (520, 3, 256, 0),
    (400, 3, 0, 1), (260, 3, 128, 0) -- the last block of the last case has four rows"""
    blk, K = gr.STAIR_BLK, gr.STAIR_K
    with forced(variant):
        for ci, (M, nb, step, diag) in enumerate(gr.STAIR):
            for fi, family in enumerate(("scaled", "cancel")):
                N = nb * blk
                A, B, C0, P, SP = gr.case(family, M, N, K)
                alpha, beta = gr.pair_of(ci, fi, variant)
                mask = gr.mask_stair(M, nb, blk, step, diag)
                c0 = np.where(mask, C0, gr.SENTINEL)
                ref, S = gr.combine(P, SP, c0, alpha, beta, mask)
                C = dev(c0, device)
                _ops.gemm_nt_stair(rows16(A, device), rows16(B, device), C, M, nb, blk, K, step, diag, alpha=alpha, beta=beta)
                inside(C, ref, S, K, 0.0, mask, c0)


# ---------------------------------------------------------------------------------------------------------------------
# 3. strides and offsets
# ---------------------------------------------------------------------------------------------------------------------
def _view(X, ld, off, fill, device, pad_rows=True):
    """X as a view with row stride ld at element offset `off` of a flat buffer of `fill`; -> (buffer, view, flat index mask)"""
    rows = gr.round_up(X.shape[0], 16) if pad_rows else X.shape[0]
    buf = torch.full((off + rows * ld + 16,), fill, dtype=F64, device=device)
    v = buf[off:off + rows * ld].view(rows, ld)[:, :X.shape[1]]
    v[:] = 0.0
    v[:X.shape[0]] = dev(X, device)
    inside_view = torch.zeros(buf.numel(), dtype=torch.bool, device=device)
    inside_view[off:off + rows * ld].view(rows, ld)[:, :X.shape[1]] = True
    return buf, v, inside_view


@pytest.mark.parametrize("lower", [0, 1])
@pytest.mark.parametrize("variant", gr.VARIANTS)
def test_strides_and_offsets(device, variant, lower):
    """lda = K + 2, ldb = K + 6, ldc = N + 3, the operands views into buffers of NaN, C a view at an odd offset into a buffer of
    the sentinel: bit-identical to the contiguous call, and nothing outside C[:M, :N] changes"""
    shapes = [(17, 33, 16), (129, 127, 144), (257, 130, 528)] if not lower else [(33, 33, 16), (130, 130, 80)]
    with forced(variant):
        for M, N, K in shapes:
            A, B, C0, _, _ = gr.case("scaled", M, N, K)
            alpha, beta = 0.37, -0.5
            want = gemm(rows16(A, device), rows16(B, device), M, N, K, alpha, beta, dev(C0, device), lower=lower)
            _, Av, _ = _view(A, K + 2, 6, float("nan"), device)
            _, Bv, _ = _view(B, K + 6, 10, float("nan"), device)
            cbuf, Cv, cin = _view(C0, N + 3, 5, gr.SENTINEL, device, pad_rows=False)
            assert Av.stride(0) == K + 2 and Bv.stride(0) == K + 6 and Cv.stride(0) == N + 3 and Cv.data_ptr() % 16 == 8
            _ops.gemm_nt(Av, Bv, M, N, K, alpha=alpha, beta=beta, C=Cv, lower=lower)
            assert same_bits(Cv, want), (M, N, K)
            assert all_bits(cbuf[~cin], gr.SENTINEL), "wrote outside C[:M, :N]"


# ---------------------------------------------------------------------------------------------------------------------
# 4. beta == 0 never reads C
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lower", [0, 1, 2])
@pytest.mark.parametrize("variant", gr.VARIANTS)
def test_beta_zero_never_reads_c(device, variant, lower):
    """C pre-filled with NaN and with Inf: the written entries are bit-identical to the call on a zeroed C (and the entries a
    lower launch leaves alone keep their fill)"""
    shapes = {0: [(17, 33, 16), (129, 127, 144)], 1: [(33, 33, 16), (130, 130, 80)], 2: [(130, 64, 48), (300, 129, 48)]}[lower]
    with forced(variant):
        for M, N, K in shapes:
            A, B, _, _, _ = gr.case("scaled", M, N, K)
            Ad, Bd = rows16(A, device), rows16(B, device)
            mask = dev(gr.mask_lower(M, N) if lower else np.ones((M, N), dtype=bool), device)
            want = gemm(Ad, Bd, M, N, K, -3.25, 0.0, torch.zeros(M, N, dtype=F64, device=device), lower=lower)
            assert torch.isfinite(want).all()
            for fill in (float("nan"), float("inf")):
                C = gemm(Ad, Bd, M, N, K, -3.25, 0.0, torch.full((M, N), fill, dtype=F64, device=device), lower=lower)
                assert same_bits(C[mask], want[mask]), (M, N, K, fill)
                assert all_bits(C[~mask], fill)


# ---------------------------------------------------------------------------------------------------------------------
# 5. padding rows, 6. propagation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", gr.VARIANTS)
def test_padding_rows_may_hold_anything(device, variant):
    """rows M..round_up(M, 16) of A and N..round_up(N, 16) of B filled with NaN: every bit equals the zero-padded call"""
    with forced(variant):
        for M, N, K in gr.SHAPES:
            A, B, C0, _, _ = gr.case("scaled", M, N, K)
            want = gemm(rows16(A, device), rows16(B, device), M, N, K, -1.0, 1.0, dev(C0, device))
            got = gemm(rows16(A, device, float("nan")), rows16(B, device, float("nan")), M, N, K, -1.0, 1.0, dev(C0, device))
            assert torch.isfinite(want).all()
            assert same_bits(got, want), (M, N, K)
        n, K = 130, 80
        A, B, C0, _, _ = gr.case("scaled", n, n, K)
        for lower in (1, 2):
            want = gemm(rows16(A, device), rows16(B, device), n, n, K, -1.0, 1.0, dev(C0, device), lower=lower)
            got = gemm(rows16(A, device, float("nan")), rows16(B, device, float("nan")), n, n, K, -1.0, 1.0, dev(C0, device), lower=lower)
            assert same_bits(got, want), lower


@pytest.mark.parametrize("planted", [float("nan"), float("inf")])
@pytest.mark.parametrize("variant", gr.VARIANTS)
def test_non_finite_values_stay_in_their_row_and_column(device, variant, planted):
    """a NaN or +Inf at A[i0, k0] makes row i0 of C non-finite (B[:, k0] has no zero) and leaves every other row's bits alone; the
    same with B[j0, k0] and column j0; i0, j0 in the last, partial tile"""
    with forced(variant):
        for M, N, K in [(65, 63, 80), (129, 127, 144), (257, 130, 528)]:
            A, B, C0, _, _ = gr.case("scaled", M, N, K)
            i0, j0, k0 = M - 1, N - 2, K - 3
            assert np.all(B[:, k0] != 0.0) and np.all(A[:, k0] != 0.0)
            Bd, Ad, Cd = rows16(B, device), rows16(A, device), dev(C0, device)
            clean = gemm(Ad, Bd, M, N, K, 0.37, -0.5, Cd)
            assert torch.isfinite(clean).all()
            A2 = A.copy()
            A2[i0, k0] = planted
            got = gemm(rows16(A2, device), Bd, M, N, K, 0.37, -0.5, Cd)
            others = torch.arange(M, device=device) != i0
            assert not torch.isfinite(got[i0]).any() and same_bits(got[others], clean[others]), (M, N, K)
            B2 = B.copy()
            B2[j0, k0] = planted
            got = gemm(Ad, rows16(B2, device), M, N, K, 0.37, -0.5, Cd)
            others = torch.arange(N, device=device) != j0
            assert not torch.isfinite(got[:, j0]).any() and same_bits(got[:, others], clean[:, others]), (M, N, K)


# ---------------------------------------------------------------------------------------------------------------------
# 7. tile-shape independence
# ---------------------------------------------------------------------------------------------------------------------
def _independence_cases(family):
    cases = [(M, N, K, 0, 0) for M, N, K in gr.SHAPES] + [(257, 257, 80, 1, 0), (130, 130, 16, 1, 0), (300, 129, 48, 2, 0),
                                                         (gr.BATCH_SHAPE + (0, 0)), (gr.BATCH_SHAPE + (1, 0))]
    out = [(gr.case(family, M, N, K)[:3], (M, N, K, lower, flags)) for M, N, K, lower, flags in cases]
    for (M, N, K), lower, flags in [((200, 72, 208), 0, UU), ((200, 200, 208), 1, UU), ((200, 72, 208), 0, gr.TRI_A_LOWER | gr.TRI_B_UPPER),
                                    ((72, 200, 208), 0, gr.TRI_B_LOWER)]:
        out.append((gr.tri_case(M, N, K, flags)[:3], (M, N, K, lower, flags)))
    return out


@pytest.mark.parametrize("family", ["scaled", "cancel"])
def test_every_tile_shape_gives_the_same_bits(device, family):
    """The lock-step and batched drivers promise results "bit-identical per model", and a batch of B models runs on another tile
    shape than one model (gemm_nt_impl chooses by tiles(b) * batch).  That holds only if every tile shape sums in the same order:
    on full-mantissa data -- where a different order WOULD show -- the three shapes of the shipped dispatch (32 x 32 ring, 64 x 64
    and 128 x 128 pipelined: variants 6, 8, 11) give the same bits, and so does every other variant (register staging, the plain
    loops, the 4-wave and 64 x 32-wave forms of the big tile): full rectangle, lower = 1, lower = 2, K-clipped operands."""
    cases = _independence_cases(family)
    results = {}
    for variant in gr.VARIANTS:
        with forced(variant):
            results[variant] = []
            for (A, B, C0), (M, N, K, lower, flags) in cases:
                C = gemm(rows16(A, device), rows16(B, device), M, N, K, 0.37, -0.5, dev(C0, device), lower=lower, tri=flags)
                results[variant].append(C)
    differ = {}
    for variant in gr.VARIANTS:
        for ci, (_, what) in enumerate(cases):
            if not same_bits(results[variant][ci], results[gr.SHIPPED[0]][ci]):
                differ.setdefault(variant, []).append(what)
    assert not any(v in differ for v in gr.SHIPPED), "the shipped tile shapes differ: %s" % {v: differ[v] for v in gr.SHIPPED if v in differ}
    assert not differ, differ


# ---------------------------------------------------------------------------------------------------------------------
# 8. K clipping of triangular operands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", gr.TRI_SHAPES)
@pytest.mark.parametrize("variant", [0, 4, 6, 8, 11])
def test_tri_flags_on_strict_triangles(device, variant, M, N, K):
    """every combination 1..15 of the GPN_TRI_* flags on operands that are strict triangles accordingly: bit-identical to the
    unclipped launch on the same operands, and within the bound.  Rectangular problems, and M > K = 144: there the A_UPPER rows
    from K on are all zero and their tiles have an EMPTY K range (as have the tiles with m0 >= n0 + BN under A_UPPER | B_LOWER) --
    zero K-steps, the tile is beta * C."""
    with forced(variant):
        for flags in range(1, 16):
            A, B, C0, P, SP = gr.tri_case(M, N, K, flags)
            alpha, beta = gr.pair_of(flags, variant)
            Ad, Bd, Cd = rows16(A, device), rows16(B, device), dev(C0, device)
            plain = gemm(Ad, Bd, M, N, K, alpha, beta, Cd)
            clipped = gemm(Ad, Bd, M, N, K, alpha, beta, Cd, tri=flags)
            assert same_bits(clipped, plain), flags
            ref, S = gr.combine(P, SP, C0, alpha, beta)
            inside(clipped, ref, S, K)


@pytest.mark.parametrize("variant", [4, 6, 8, 11])
@pytest.mark.parametrize("flag", [gr.TRI_A_LOWER, gr.TRI_B_LOWER])
def test_lower_flags_need_a_strict_triangle(device, variant, flag):
    """gpnative.h: a *_LOWER operand must be zero for EVERY k > i, not merely from the next multiple of 128 on.  The kernel
    clips the K range at the edge of its own tile, 32, 64 or 128 rows by the launch: an operand that is dense up to the next 128
    boundary gives exactly the product of its part left of k = b ceil((i + 1) / b) for b x b tiles -- bit for bit the unclipped
    launch on that part -- so on 32- and 64-row tiles (which the shipped dispatch picks below 64 tiles) terms are missing."""
    M = N = 200
    K = 208
    b = gr.TILE_EDGE[variant]
    X = gr.dense_to_edge(M, K, 128)
    Y = gr.scaled(N, N, K, salt=3)[0]
    Xc = gr.clip_to_tile(X, b)
    A, B, Ac, Bc = (X, Y, Xc, Y) if flag == gr.TRI_A_LOWER else (Y, X, Y, Xc)
    zero = torch.zeros(M, N, dtype=F64, device=device)
    with forced(variant):
        got = gemm(rows16(A, device), rows16(B, device), M, N, K, 1.0, 0.0, zero, tri=flag)
        want = gemm(rows16(Ac, device), rows16(Bc, device), M, N, K, 1.0, 0.0, zero)
    assert same_bits(got, want)
    ref, S = gr.ref_nt(A, B)                                          # the product of the operand as passed
    lost = np.abs(gr.ld(got.cpu().numpy()) - ref) > gr.bound(K, S)
    assert lost.any() == (b < 128)


# ---------------------------------------------------------------------------------------------------------------------
# 9. thin tiles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", gr.THIN_SHAPES)
@pytest.mark.parametrize("variant", (0,) + PIPELINED)
def test_thin_tiles(device, variant, M, N, K):
    """a last tile row with at most 16 rows of the matrix skips the MFMAs of its empty blocks (the pipelined tile shapes): the
    same bits with the path off and on, within the bound"""
    A, B, C0, P, SP = gr.case("scaled", M, N, K)
    alpha, beta = gr.pair_of(M, variant)
    out = []
    for thin in (0, 1):
        with forced(variant, thin):
            out.append(gemm(rows16(A, device), rows16(B, device), M, N, K, alpha, beta, dev(C0, device)))
    assert same_bits(out[0], out[1])
    ref, S = gr.combine(P, SP, C0, alpha, beta)
    inside(out[1], ref, S, K)


# ---------------------------------------------------------------------------------------------------------------------
# 10. batched forms
# ---------------------------------------------------------------------------------------------------------------------
def _batch_operands(shape, batch, device):
    M, N, K = shape
    mp, np_ = gr.round_up(M, 16), gr.round_up(N, 16)
    A = torch.zeros(batch * mp, K, dtype=F64, device=device)
    B = torch.zeros(batch * np_, K, dtype=F64, device=device)
    C0 = torch.empty(batch, M, N, dtype=F64, device=device)
    host = []
    for z in range(batch):
        a, b, c = gr.scaled(M, N, K, salt=10 + z)
        A[z * mp:z * mp + M], B[z * np_:z * np_ + N], C0[z] = dev(a, device), dev(b, device), dev(c, device)
        host.append((a, b, c))
    return A, B, C0, mp, np_, host


@pytest.mark.parametrize("lower", [0, 1])
@pytest.mark.parametrize("batch", [1, 3, 5])
@pytest.mark.parametrize("variant", (0,) + gr.SHIPPED)
def test_batched_matches_single_launches(device, variant, batch, lower):
    """gpn_gemm_nt_batched with distinct operands per problem: each problem is bit-identical to its own gpn_gemm_nt call.  Under
    the shipped dispatch (variant 0) one 200 x 200 problem runs on 32 x 32 tiles and five of them on 64 x 64."""
    for shape in (gr.BATCH_SHAPE, (33, 33, 16)):
        M, N, K = shape
        A, B, C0, mp, np_, host = _batch_operands(shape, batch, device)
        with forced(variant):
            C = C0.clone()
            _ops.gemm_nt_batched(A, B, M, N, K, batch, mp * K, np_ * K, C, alpha=0.37, beta=-0.5, lower=bool(lower))
            for z in range(batch):
                single = gemm(A[z * mp:(z + 1) * mp], B[z * np_:(z + 1) * np_], M, N, K, 0.37, -0.5, C0[z], lower=lower)
                assert same_bits(C[z], single), (shape, z)
        a, b, c = host[batch - 1]
        mask = gr.mask_lower(M, N) if lower else np.ones((M, N), dtype=bool)
        ref, S = gr.ref_nt(a, b, c, 0.37, -0.5, mask)
        inside(C[batch - 1], ref, S, K, 0.0, mask, c)


@pytest.mark.parametrize("variant", (0,) + gr.SHIPPED)
def test_batched_split_k(device, variant):
    """the split-K form of gpnative.h: sA = sB = K over ONE set of rows, five parts of 48 columns; the partial results sum to the
    reference within the sum of the parts' bounds, (48 + 3) 2^-53 S of the whole product"""
    M, N, K, parts = gr.SPLITK
    A, B, _ = gr.scaled(M, N, K * parts, salt=5)
    C = torch.full((parts, M, N), float("nan"), dtype=F64, device=device)
    with forced(variant):
        _ops.gemm_nt_batched(rows16(A, device), rows16(B, device), M, N, K, parts, K, K, C)
    total = np.sum(gr.ld(C.cpu().numpy()), axis=0)
    ref, S = gr.ref_nt(A, B)
    assert np.all(np.abs(total - ref) <= gr.bound(K, S))
    z = 3                                                           # and one part on its own
    refz, Sz = gr.ref_nt(A[:, z * K:(z + 1) * K], B[:, z * K:(z + 1) * K])
    inside(C[z], refz, Sz, K)


@pytest.mark.parametrize("lower", [0, 1])
@pytest.mark.parametrize("variant", (0,) + gr.SHIPPED)
def test_batched_scaled_matches_single_launches(device, variant, lower):
    """gpn_gemm_nt_batched_scaled, the scales in device memory (a negative one and 2^-30 among them): each problem bit-identical
    to gpn_gemm_nt(alpha = alphas[z]), as gpnative.h promises"""
    alphas_h = [0.37, -1.5, 2.0 ** -30, 1.0, -3.25]
    for shape, batch in ((gr.BATCH_SHAPE, 5), (gr.BATCH_SHAPE, 1), ((33, 33, 16), 3)):
        M, N, K = shape
        A, B, C0, mp, np_, host = _batch_operands(shape, batch, device)
        alphas = torch.tensor(alphas_h[:batch], dtype=F64, device=device)
        with forced(variant):
            C = C0.clone()
            _ops.gemm_nt_batched_scaled(A, B, M, N, K, batch, mp * K, np_ * K, C, alphas, beta=-0.5, lower=bool(lower))
            for z in range(batch):
                single = gemm(A[z * mp:(z + 1) * mp], B[z * np_:(z + 1) * np_], M, N, K, alphas_h[z], -0.5, C0[z], lower=lower)
                assert same_bits(C[z], single), (shape, batch, z)
        z = batch - 1
        a, b, c = host[z]
        mask = gr.mask_lower(M, N) if lower else np.ones((M, N), dtype=bool)
        ref, S = gr.ref_nt(a, b, c, alphas_h[z], -0.5, mask)
        inside(C[z], ref, S, K, 0.0, mask, c)


def test_batched_scaled_validation(device):
    """-4 for K = 0 (and K % 16), -5 for NULL alphas, -17 for tri outside 0..15, -18 for batch < 1: returned before any launch,
    C untouched"""
    M, N, K = 33, 18, 16
    A, B, C = (torch.ones(48, K, dtype=F64, device=device), torch.ones(32, K, dtype=F64, device=device),
               torch.full((M, N), gr.SENTINEL, dtype=F64, device=device))
    alphas = torch.ones(1, dtype=F64, device=device)
    lib = _native.lib()

    def call(K_=K, alphas_=alphas, tri=0, batch=1):
        return lib.gpn_gemm_nt_batched_scaled(_ops._stream(device), M, N, K_, _ops._ptr(alphas_), _ops._ptr(A), K, 48 * K, _ops._ptr(B), K, 32 * K,
                                              0.0, _ops._ptr(C), N, M * N, 0, tri, batch)
    assert call(K_=0) == -4 and call(K_=8) == -4
    assert call(alphas_=None) == -5
    assert call(tri=16) == -17 and call(tri=-1) == -17
    assert call(batch=0) == -18
    torch.cuda.synchronize()
    assert all_bits(C, gr.SENTINEL)
    assert call() == 0
    torch.cuda.synchronize()
    assert same_bits(C, torch.full_like(C, float(K)))


# ---------------------------------------------------------------------------------------------------------------------
# 11. _ops.matmul_nt, K = 0
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", gr.MATMUL_K + (48,))
def test_matmul_nt_repacks_what_the_kernel_cannot_take(device, K):
    """K no multiple of 16, views at an odd (8-byte aligned) offset, a non-contiguous B: all within bound(K, S)"""
    M, N = (32, 16) if K == 48 else (33, 18)
    A, B, _ = gr.scaled(M, N, K)
    ref, S = gr.ref_nt(A, B, None, -0.75, 0.0)
    Ad, Bd = dev(A, device), dev(B, device)
    inside(_ops.matmul_nt(Ad, Bd, alpha=-0.75), ref, S, K)
    odd = []
    for X in (A, B):
        buf = torch.full((X.size + 3,), float("nan"), dtype=F64, device=device)
        v = buf[1:1 + X.size].view(X.shape)
        v[:] = dev(X, device)
        assert v.data_ptr() % 16 == 8
        odd.append(v)
    inside(_ops.matmul_nt(odd[0], odd[1], alpha=-0.75), ref, S, K)
    Bt = dev(B.T, device)                                        # [K, N] contiguous: its transpose has stride (1, N)
    assert K == 1 or not Bt.t().is_contiguous()
    inside(_ops.matmul_nt(Ad, Bt.t(), alpha=-0.75), ref, S, K)
    inside(_ops.matmul_nt(odd[0], Bt.t(), alpha=-0.75), ref, S, K)


def test_k_zero_is_unsupported(device):
    """gpn_gemm_nt with K = 0 (C = beta C) returns GPN_E_UNSUPPORTED and writes nothing"""
    A, B = torch.ones(16, 16, dtype=F64, device=device), torch.ones(16, 16, dtype=F64, device=device)
    C = torch.full((16, 16), gr.SENTINEL, dtype=F64, device=device)
    st = _native.lib().gpn_gemm_nt(_ops._stream(device), 16, 16, 0, 1.0, _ops._ptr(A), 16, _ops._ptr(B), 16, 0.5, _ops._ptr(C), 16, 0, 0)
    assert st == -102
    torch.cuda.synchronize()
    assert all_bits(C, gr.SENTINEL)
