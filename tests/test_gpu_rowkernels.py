"""The row kernels of the sparse models (csrc/svgp.hip, csrc/fitc.hip and the tile pass they share, csrc/rowkernels.h) called
through the C ABI, one kernel at a time, against the long-double statement of include/gpnative.h's promises (tests/_rowref.py)
-- at the tile and width edges that no model of the suite reaches:

    rows  m     dy   reaches
    1     2     1    the smallest legal shape
    1     1     1    lda = ldt = 2
    15    5     1
    16    64    4    an exact tile, an exact SV_DYB pass
    17    65    5    a second column tile one column wide, a second SV_DYB pass
    33    63    8    a third 16-row group, exactly one RK_GB staging
    31    127   9
    47    129   17   three RK_GB stagings
    50    1023  2
    32    1024  3    the last m of fitc_forward_rows_kernel<8>
    18    1025  3    fitc_forward_rows_kernel<32>, the second SV_JT tile of the marginals, odd m
    35    1026  65   the k += 64 lane loops over dy of both FITC kernels
    20    4096  1    the last m held in registers
    20    4097  2    the re-read tail loops of the FITC forward, odd m
    19    4225  8    67 column tiles

Every shape runs under all 16 layouts: kdiag_stride 0 / 1, ldw = ldb = dy / dy + 3, the leading dimensions of alpha and T at
their tightest legal value (even, with a padding column) / at the models' (round_up(m, 128); FITC's T: round_up(m, 16) +
round_up(dy, 16)), ldo = round_up(rows, 16) / larger.

POISON.  Every buffer, input or output, is a window into a larger allocation filled with NaNs whose payload is the buffer's tag
and the entry's position; real values are written only where the header says the kernel reads.  So a kernel that reads a padding
column, a padding row or a neighbour's entry produces a NaN, and one that writes anything anywhere outside its documented
outputs -- even a copy of some other poison -- changes bits that are compared with a snapshot taken before the call.

TOLERANCE.  tests/_xref.tol's rule with the suite's tightest floor: max(16 e64, 1e-13) on max |got - ref| / max(1, max |ref|),
where e64 is the error of the SAME reference run in float64 against its long-double run, per case and per output: computed from
the reference alone, never from the kernel.  With these continuous random inputs one dropped or doubled term moves an output by
far more than that at every shape (the smallest terms, alpha_ij^2 at m = 4225, are ~1e-4)."""
import functools
import itertools

import numpy as np
import pytest
import torch

from gptorch_amd import _native, _ops
from tests import _rowref as rr
from tests import _xref as xr

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 1), (1, 1, 1), (15, 5, 1), (16, 64, 4), (17, 65, 5), (33, 63, 8), (31, 127, 9), (47, 129, 17), (50, 1023, 2), (32, 1024, 3),
          (18, 1025, 3), (35, 1026, 65), (20, 4096, 1), (20, 4097, 2), (19, 4225, 8)]
IDS = ["%dx%dx%d" % s for s in SHAPES]
# (kdiag_stride, ldw - dy = ldb - dy, leading dimensions of alpha / T, ldo - round_up(rows, 16))
LAYOUTS = list(itertools.product((0, 1), (0, 3), ("tight", "model"), (0, 6)))
FLOOR = xr.FLOOR["K"]                                                          # 1e-13, the tightest floor of the suite
GPN_OK = 0
MARGIN = 64                                                                   # doubles of canary on either side (even: 16-byte aligned)
NAN_BITS = 0x7FF8000000000000


def ld_of(m, how):
    """alpha / T [rows, m]: the tightest even leading dimension that leaves a padding column, or the models'."""
    return (m + 2 if m % 2 == 0 else m + 1) if how == "tight" else rr.round_up(m, 128)


def ldt_fitc(m, dy, how):
    mp = rr.round_up(m, 16)
    return rr.round_up(mp + dy, 2) if how == "tight" else mp + rr.round_up(dy, 16)


class Buf:
    """a [rows, ld] window into a larger allocation of NaNs, each with its own payload (tag, position)."""

    def __init__(self, device, tag, rows, ld):
        n = 2 * MARGIN + rows * ld
        self.flat = (torch.arange(1, n + 1, dtype=torch.int64, device=device) + (NAN_BITS + (tag << 32))).view(torch.float64)
        self.mat = self.flat[MARGIN:MARGIN + rows * ld].view(rows, ld)
        self.shape = (rows, ld)
        self.written = np.zeros((rows, ld), dtype=bool)                       # what the header lets the kernel write
        self.before = None

    def put(self, a, c0=0):
        a = np.asarray(a, dtype=np.float64)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        self.mat[:a.shape[0], c0:c0 + a.shape[1]] = torch.as_tensor(a, device=self.flat.device)
        return self

    def out(self, rows, cols):
        self.written[:rows, :cols] = True
        return self

    @property
    def ptr(self):
        return _ops._ptr(self.mat)

    def bits(self, t):
        return t.cpu().numpy().view(np.int64)

    def fetch(self):
        """after the call: -> the window on the host; asserts that nothing outside `written` changed, canaries included."""
        before, after = self.bits(self.before), self.bits(self.flat)
        keep = np.ones(before.size, dtype=bool)
        keep[MARGIN:before.size - MARGIN] = ~self.written.ravel()
        bad = np.nonzero(keep & (before != after))[0]
        assert bad.size == 0, "wrote outside the documented region: %d entries, first at window offset %d of a %s window" % (
            bad.size, bad[0] - MARGIN, self.shape)
        return self.flat.cpu().numpy()[MARGIN:before.size - MARGIN].reshape(self.shape)


def launch(device, bufs, call):
    """snapshot, call, synchronise -> return code."""
    for b in bufs.values():
        b.before = b.flat.clone()
    torch.cuda.synchronize(device)
    rc = call(_native.lib(), _ops._stream(device))
    torch.cuda.synchronize(device)
    return rc


def is_zero_bits(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.int64) == 0))          # +0.0, bit for bit (not -0.0)


@functools.lru_cache(maxsize=None)
def case(rows, m, dy):
    """inputs and, per kernel (and per kdiag variant where kdiag enters), the long-double outputs with their tolerances; built once
    per shape, shared by the tests and never modified."""
    d = rr.inputs(rows, m, dy)
    calls = {
        ("marginals", 1): (rr.svgp_marginals, (d["alpha"], d["T"], d["w"], d["kdiag"])),
        ("marginals", 0): (rr.svgp_marginals, (d["alpha"], d["T"], d["w"], d["kdiag_shared"])),
        ("svgp_backward", None): (rr.svgp_backward_rows, (d["alpha"], d["T"], d["w"], d["g_var"], d["g_mean"])),
        ("fitc_forward", 1): (rr.fitc_forward_rows, (d["At_fwd"], d["err"], d["kdiag_fwd"], d["noise"])),
        ("fitc_forward", 0): (rr.fitc_forward_rows, (d["At_fwd"], d["err"], d["kdiag_shared"], d["noise"])),
        ("fitc_backward", None): (rr.fitc_backward_rows, (d["alpha"], d["Tf"], m, d["beta"], d["err"], d["lam"])),
    }
    refs = {}
    for key, (fn, args) in calls.items():
        hi, lo = fn(*args, dtype=rr.LD), fn(*args, dtype=np.float64)
        refs[key] = {k: (hi[k], max(xr.SAFETY * xr.rel_err(lo[k], hi[k]), FLOOR), xr.rel_err(lo[k], hi[k])) for k in hi}
    return d, refs


class Report:
    """the worst observed error of each output over the layouts of a test, next to its e64 and tolerance (printed: LAB.md)."""

    def __init__(self, name, shape):
        self.name, self.shape, self.worst = name, shape, {}

    def check(self, ref, key, got, layout):
        want, tol, e64 = ref[key]
        got = np.asarray(got)
        assert got.shape == want.shape and np.all(np.isfinite(got)), (self.name, key, layout)
        err = xr.rel_err(got, want)
        self.worst[key] = max(self.worst.get(key, 0.0), err)
        assert err <= tol, "%s %s %s layout %s: err %.3e > tol %.3e (e64 %.1e)" % (self.name, self.shape, key, layout, err, tol, e64)

    def show(self, ref):
        print("%s %s: " % (self.name, self.shape) + "  ".join("%s err %.1e (e64 %.1e, tol %.1e)" % (k, v, ref[k][2], ref[k][1])
                                                              for k, v in self.worst.items()))


def same_bits(first, second):
    for name in first:
        a, b = first[name], second[name]
        assert np.array_equal(a.bits(a.flat), b.bits(b.flat)), "a second call on fresh copies gave other bits in " + name


def kdiag_buf(device, tag, d, key, kds):
    return Buf(device, tag, 1, len(d[key])).put(d[key]) if kds else Buf(device, tag, 1, 1).put(d["kdiag_shared"][:1])


def transposed_outputs(device, tags, m, ldo, rpad):
    """alphaT / galphaT [m, ldo] with a poisoned row below them: written in rows < m, columns < round_up(rows, 16)."""
    return [Buf(device, t, m + 1, ldo).out(m, rpad) for t in tags]


def check_transposed(rep, ref, layout, bufs, rows, rpad, m):
    for name in ("alphaT", "galphaT"):
        got = bufs[name].fetch()
        rep.check(ref, name, got[:m, :rows], layout)
        assert is_zero_bits(got[:m, rows:rpad]), (name, layout)                # the contractions' K padding: exact zeros


# ---- gpn_svgp_marginals ----------------------------------------------------------------------------------------------------
def run_marginals(device, d, rows, m, dy, layout):
    kds, dw, how, _ = layout
    lda = ldt = ld_of(m, how)
    bufs = dict(alpha=Buf(device, 1, rows, lda).put(d["alpha"]), T=Buf(device, 2, rows, ldt).put(d["T"]),
                w=Buf(device, 3, m, dy + dw).put(d["w"]), kdiag=kdiag_buf(device, 4, d, "kdiag", kds),
                f_mean=Buf(device, 5, rows, dy).out(rows, dy), f_var=Buf(device, 6, 1, rows).out(1, rows))
    b = bufs
    rc = launch(device, bufs, lambda lib, s: lib.gpn_svgp_marginals(s, b["alpha"].ptr, lda, b["T"].ptr, ldt, rows, m, b["w"].ptr, dy + dw, dy,
                                                                   b["kdiag"].ptr, kds, b["f_mean"].ptr, b["f_var"].ptr))
    assert rc == GPN_OK, (rc, layout)
    return bufs


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_svgp_marginals(device, shape):
    rows, m, dy = shape
    d, refs = case(*shape)
    rep = Report("gpn_svgp_marginals", shape)
    for layout in LAYOUTS:
        ref = refs[("marginals", layout[0])]
        bufs = run_marginals(device, d, rows, m, dy, layout)
        got = {k: b.fetch() for k, b in bufs.items()}                          # (inputs: nothing written at all)
        rep.check(ref, "f_mean", got["f_mean"], layout)
        rep.check(ref, "f_var", got["f_var"][0], layout)
        same_bits(bufs, run_marginals(device, d, rows, m, dy, layout))
    rep.show(ref)


# ---- gpn_svgp_backward_rows ------------------------------------------------------------------------------------------------
def run_svgp_backward(device, d, rows, m, dy, layout):
    _, dw, how, do = layout
    lda = ldt = ld_of(m, how)
    rpad = rr.round_up(rows, 16)
    ldo = rpad + do
    aT, gaT = transposed_outputs(device, (7, 8), m, ldo, rpad)
    bufs = dict(alpha=Buf(device, 1, rows, lda).put(d["alpha"]), T=Buf(device, 2, rows, ldt).put(d["T"]).out(rows, m),
                w=Buf(device, 3, m, dy + dw).put(d["w"]), g_var=Buf(device, 4, 1, rows).put(d["g_var"]),
                g_mean=Buf(device, 5, rows, dy).put(d["g_mean"]), alphaT=aT, galphaT=gaT)
    b = bufs
    rc = launch(device, bufs, lambda lib, s: lib.gpn_svgp_backward_rows(s, b["alpha"].ptr, lda, b["T"].ptr, ldt, rows, m, b["w"].ptr, dy + dw, dy,
                                                                       b["g_var"].ptr, b["g_mean"].ptr, aT.ptr, gaT.ptr, ldo))
    assert rc == GPN_OK, (rc, layout)
    return bufs


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_svgp_backward_rows(device, shape):
    rows, m, dy = shape
    d, refs = case(*shape)
    ref = refs[("svgp_backward", None)]
    rep = Report("gpn_svgp_backward_rows", shape)
    for layout in LAYOUTS:
        bufs = run_svgp_backward(device, d, rows, m, dy, layout)
        for k in ("alpha", "w", "g_var", "g_mean"):
            bufs[k].fetch()
        rep.check(ref, "T", bufs["T"].fetch()[:, :m], layout)                  # (fetch: columns >= m keep their bits)
        check_transposed(rep, ref, layout, bufs, rows, rr.round_up(rows, 16), m)
        same_bits(bufs, run_svgp_backward(device, d, rows, m, dy, layout))
    rep.show(ref)


# ---- gpn_fitc_forward_rows -------------------------------------------------------------------------------------------------
def run_fitc_forward(device, d, rows, m, dy, layout):
    kds, _, how, do = layout
    lda = ld_of(m, how)
    rpad = rr.round_up(rows, 16)
    ldo = rpad + do
    nwork = int(_native.lib().gpn_fitc_forward_work_bytes(rows)) // 8
    At = Buf(device, 1, rpad + 1, lda).put(d["At_fwd"]).out(rpad, m)           # the buffer holds round_up(rows, 16) rows; one more of poison
    if m % 2:
        # The kernel zeroes its padding rows with 16-byte stores (column pairs), so for odd m the last store of a padding row
        # covers column m, a padding column of a padding row that nothing reads: it may hold its poison or 0.0.  (Column m of
        # a REAL row is written with an 8-byte store and must keep its poison.)
        At.written[rows:rpad, m] = True
    bufs = dict(At=At, err=Buf(device, 2, rows, dy).put(d["err"]), kdiag=kdiag_buf(device, 3, d, "kdiag_fwd", kds),
                errT=Buf(device, 4, dy + 1, ldo).out(dy, rpad), lam=Buf(device, 5, 1, rows).out(1, rows),
                work=Buf(device, 6, 1, nwork).out(1, nwork), out2=Buf(device, 7, 1, 2).out(1, 2))
    b = bufs
    rc = launch(device, bufs, lambda lib, s: lib.gpn_fitc_forward_rows(s, At.ptr, lda, rows, m, b["err"].ptr, dy, b["kdiag"].ptr, kds, d["noise"],
                                                                      b["errT"].ptr, ldo, b["lam"].ptr, b["work"].ptr, b["out2"].ptr))
    assert rc == GPN_OK, (rc, layout)
    return bufs


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fitc_forward_rows(device, shape):
    rows, m, dy = shape
    d, refs = case(*shape)
    rpad = rr.round_up(rows, 16)
    rep = Report("gpn_fitc_forward_rows", shape)
    for layout in LAYOUTS:
        ref = refs[("fitc_forward", layout[0])]
        bufs = run_fitc_forward(device, d, rows, m, dy, layout)
        bufs["err"].fetch(), bufs["kdiag"].fetch(), bufs["work"].fetch()
        At, errT = bufs["At"].fetch(), bufs["errT"].fetch()
        rep.check(ref, "lam", bufs["lam"].fetch()[0], layout)
        rep.check(ref, "At", At[:rows, :m], layout)
        rep.check(ref, "errT", errT[:dy, :rows], layout)
        rep.check(ref, "out2", bufs["out2"].fetch()[0], layout)
        assert is_zero_bits(At[rows:rpad, :m]) and is_zero_bits(errT[:dy, rows:rpad]), layout
        if m % 2:                                                              # the allowance above: poison or 0.0, nothing else
            before = bufs["At"].bits(bufs["At"].before)[MARGIN:-MARGIN].reshape(At.shape)[rows:rpad, m]
            after = np.ascontiguousarray(At[rows:rpad, m]).view(np.int64)
            assert np.all((after == before) | (after == 0)), layout
        same_bits(bufs, run_fitc_forward(device, d, rows, m, dy, layout))
    rep.show(ref)
    lam = bufs["lam"].fetch()[0]
    assert all(lam[i] == d["noise"] for i in d["cancel"])                      # the cancellation rows: lambda is the noise, exactly


# ---- gpn_fitc_backward_rows ------------------------------------------------------------------------------------------------
def run_fitc_backward(device, d, rows, m, dy, layout):
    _, dw, how, do = layout
    lda, ldt = ld_of(m, how), ldt_fitc(m, dy, how)
    mp, rpad = rr.round_up(m, 16), rr.round_up(rows, 16)
    ldo = rpad + do
    aT, gaT = transposed_outputs(device, (9, 10), m, ldo, rpad)
    T = Buf(device, 2, rows, ldt).put(d["Tf"][:, :m]).put(d["Tf"][:, mp:], c0=mp).out(rows, m)   # columns m .. mp - 1 and >= mp + dy: poison
    bufs = dict(alpha=Buf(device, 1, rows, lda).put(d["alpha"]), T=T, beta=Buf(device, 3, m, dy + dw).put(d["beta"]),
                err=Buf(device, 4, rows, dy).put(d["err"]), lam=Buf(device, 5, 1, rows).put(d["lam"]),
                r=Buf(device, 6, rows, dy).out(rows, dy), g=Buf(device, 7, 1, rows).out(1, rows), alphaT=aT, galphaT=gaT)
    b = bufs
    rc = launch(device, bufs, lambda lib, s: lib.gpn_fitc_backward_rows(s, b["alpha"].ptr, lda, T.ptr, ldt, rows, m, b["beta"].ptr, dy + dw, dy,
                                                                       b["err"].ptr, b["lam"].ptr, b["r"].ptr, b["g"].ptr, aT.ptr, gaT.ptr, ldo))
    assert rc == GPN_OK, (rc, layout)
    return bufs


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fitc_backward_rows(device, shape):
    rows, m, dy = shape
    d, refs = case(*shape)
    ref = refs[("fitc_backward", None)]
    rep = Report("gpn_fitc_backward_rows", shape)
    for layout in LAYOUTS:
        bufs = run_fitc_backward(device, d, rows, m, dy, layout)
        for k in ("alpha", "beta", "err", "lam"):
            bufs[k].fetch()
        rep.check(ref, "r", bufs["r"].fetch(), layout)
        rep.check(ref, "g", bufs["g"].fetch()[0], layout)
        rep.check(ref, "T", bufs["T"].fetch()[:, :m], layout)                  # (fetch: the alpha beta block and the padding keep their bits)
        check_transposed(rep, ref, layout, bufs, rows, rr.round_up(rows, 16), m)
        same_bits(bufs, run_fitc_backward(device, d, rows, m, dy, layout))
    rep.show(ref)


def test_the_poison_is_nan_everywhere_and_distinct(device):
    """the harness itself: every poison entry is a NaN, no two buffers or positions share bits, and fetch() sees a changed bit."""
    a, b = Buf(device, 1, 3, 4), Buf(device, 2, 3, 4)
    assert bool(torch.isnan(a.flat).all()) and bool(torch.isnan(b.flat).all())
    bits = np.concatenate([a.bits(a.flat), b.bits(b.flat)])
    assert np.unique(bits).size == bits.size
    a.out(2, 3).put(np.ones((2, 3)))
    a.before = a.flat.clone()
    a.mat[:2, :3] = 2.0
    assert np.array_equal(a.fetch()[:2, :3], np.full((2, 3), 2.0))
    a.mat[2, 3] = a.mat[2, 2]                                                  # a copy of a neighbour's poison
    with pytest.raises(AssertionError, match="outside the documented region"):
        a.fetch()
    a.before = a.flat.clone()
    a.flat[MARGIN - 1] = 0.0                                                   # the canary
    with pytest.raises(AssertionError, match="outside the documented region"):
        a.fetch()
