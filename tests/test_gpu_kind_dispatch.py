"""Every entry point of include/gpnative.h that takes a kernel kind, run with every kind 0 .. 5 and with -1 and 6 on one small
shape (tests/_kind_ref.py: n = 65, m = 63, d = 2, ARD, dy = 2, batch = 3); the ragged LML forms, which take more than 256 rows,
on two models of 289 and 257 points.

  kind served      the output meets THAT kind's long-double reference at xr.tol(e64, what), e64 from the fp64 host statement of
                   the same sums; a lock-step form is also bit-identical, slot by slot, to its single call.
  kind not served  a negative status, and after a device synchronisation every output and workspace buffer still holds its
                   sentinel bit for bit (the points it would have read are NaN).

tests/test_kind_ref_host.py shows that the kinds' references lie a million tolerances apart on these inputs: an entry that ran
another kind's instantiation -- a swapped case label, a kind falling into a switch's default -- fails here."""
import ctypes

import numpy as np
import pytest
import torch

from gptorch_amd import _native
from tests import _kind_ref as kr
from tests import _xref as xr

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
ISENTINEL = -77
ALL_KINDS = kr.KIND_IDS + kr.BAD_KINDS


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Ctx:
    """the inputs on the device, and the buffers of ONE call: outputs and workspaces start as sentinels."""

    def __init__(self, device):
        inp = kr.inputs()
        self.inp, self.dev, self.lib = inp, device, _native.lib()
        t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=device)
        self.X, self.X2, self.Y = t(inp.X), t(inp.X2), t(inp.Y)
        self.Xnan, self.X2nan = torch.full_like(self.X, float("nan")), torch.full_like(self.X2, float("nan"))
        self.var, self.ls, self.noise = t(inp.var), t(inp.ls), t(inp.noise)
        self.G, self.P, self.at, self.wt, self.s, self.vec = t(inp.G), t(inp.P), t(inp.at), t(inp.wt), t(inp.s), t(inp.vec)
        # the lower triangle is what the sweeps read: NaN above it
        self.Plow = torch.tril(self.P) + torch.triu(torch.full_like(self.P, float("nan")), 1)
        self.n, self.m, self.d, self.dy, self.B = inp.n, inp.m, inp.d, inp.dy, inp.batch
        self.lda = int(self.lib.gpn_factor_ld(self.n, self.dy))
        self.rows = int(self.lib.gpn_factor_rows(self.n, self.dy))
        self.sA = self.rows * self.lda
        self.sW = int(self.lib.gpn_winv_bytes(self.n)) // 8
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        self.bufs = []
        self._factors = {}

    def buf(self, *shape, zero=False, dtype=torch.float64):
        """an output or workspace of the call under test (zero: a buffer the entry wants zero-initialised -- still a sentinel
        when the call is expected to be refused, see `refused`)."""
        fill = ISENTINEL if dtype == torch.int32 else SENTINEL
        b = torch.full(shape, 0 if (zero and not self.poison) else fill, dtype=dtype, device=self.dev)
        if self.poison:
            self.bufs.append((b, fill))
        return b

    def work(self, nbytes, batch=1):
        return self.buf(max(1, batch * int(nbytes) // 8))

    def begin(self, served):
        self.poison = not served
        self.bufs = []
        return (self.X, self.X2) if served else (self.Xnan, self.X2nan)

    def assert_untouched(self):
        torch.cuda.synchronize()
        for b, fill in self.bufs:
            assert bool((b == fill).all()), "a refused call wrote %d entries of a buffer of shape %s" % (int((b != fill).sum()), tuple(b.shape))

    # a factor of model b (or of all models, lock-step layout) for the entries that start from one
    def factor(self, kind, b=None):
        key = (kind, b)
        if key not in self._factors:
            lib, B = self.lib, (1 if b is not None else self.B)
            A = torch.zeros(B, self.rows, self.lda, dtype=torch.float64, device=self.dev)
            winv = torch.zeros(B, self.sW, dtype=torch.float64, device=self.dev)
            info = torch.zeros(B, dtype=torch.int32, device=self.dev)
            out3 = torch.zeros(B, 3, dtype=torch.float64, device=self.dev)
            if b is not None:
                st = lib.gpn_lml_forward(self.stream, kind, _p(self.X), self.n, self.d, _p(self.Y), None, self.dy, _p(self.var[b:]),
                                         _p(self.ls[b]), self.d, _p(self.noise[b:]), _p(A), self.lda, _p(winv), _p(info), _p(out3))
            else:
                st = lib.gpn_lml_forward_batched(self.stream, kind, B, _p(self.X), 0, self.n, self.d, _p(self.Y), 0, None, 0, self.dy,
                                                 _p(self.var), _p(self.ls), self.d, _p(self.noise), _p(A), self.lda, self.sA, _p(winv),
                                                 self.sW, _p(info), _p(out3))
            assert st == 0 and int(info.abs().max()) == 0, (st, info)
            self._factors[key] = (A, winv, info, out3)
        return self._factors[key]


@pytest.fixture(scope="module")
def ctx(device):
    return Ctx(device)


def check(family, kind, b, got):
    """every output in `got` against model b's long-double reference for THIS kind."""
    ref = kr.reference(family, kind, b)
    for name, value in got.items():
        want, tol, how = ref[name]
        v = value.detach().cpu().numpy().reshape(np.shape(want))
        err = kr.metric(v, want, how)
        print("%s %s b %d %s: err %.2e tol %.1e (err / tol %.3f)" % (family, kr.KIND_NAMES[kind], b, name, err, tol, err / tol))
        assert err <= tol, (family, kr.KIND_NAMES[kind], b, name, err, tol)


def refused(c, st):
    assert st < 0, "status %d for a kind the entry does not serve" % st
    c.assert_untouched()


def served(entry, kind):
    return kind in kr.SERVED[entry]


# ---- K assembly ------------------------------------------------------------------------------------------------------------------------
def call_kernel_matrix(c, kind, X, X2, b):
    K = c.buf(c.n, c.m)
    st = c.lib.gpn_kernel_matrix(c.stream, kind, _p(X), c.n, _p(X2), c.m, c.d, _p(c.var[b:]), _p(c.ls[b]), c.d, None, 0, _p(K), c.m)
    return st, K


def call_kernel_matrix_batched(c, kind, X, X2):
    K = c.buf(c.B, c.n, c.m)
    st = c.lib.gpn_kernel_matrix_batched(c.stream, kind, c.B, _p(X), 0, c.n, _p(X2), 0, c.m, c.d, _p(c.var), _p(c.ls), c.d, None, 0,
                                         _p(K), c.m, c.n * c.m)
    return st, K


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_kernel_matrix(ctx, kind):
    c = ctx
    ok = served("gpn_kernel_matrix", kind)
    assert ok == served("gpn_kernel_matrix_batched", kind)
    X, X2 = c.begin(ok)
    st, K = call_kernel_matrix(c, kind, X, X2, 1)
    stb, Kb = call_kernel_matrix_batched(c, kind, X, X2)
    if not ok:
        return refused(c, max(st, stb))
    assert st == 0 and stb == 0
    check("kernel_matrix", kind, 1, {"K": K})
    for b in range(c.B):
        check("kernel_matrix", kind, b, {"K": Kb[b]})
        assert torch.equal(Kb[b], call_kernel_matrix(c, kind, X, X2, b)[1])


# ---- the dense sweeps --------------------------------------------------------------------------------------------------------------------
def call_kernel_grad(c, kind, X, X2, b):
    out = c.buf(1 + c.d)
    work = c.work(c.lib.gpn_grad_work_bytes(c.n, c.m, c.d, 0))
    st = c.lib.gpn_kernel_grad(c.stream, kind, _p(X), c.n, _p(X2), c.m, c.d, _p(c.var[b:]), _p(c.ls[b]), c.d, _p(c.G[b]), c.m, _p(work), _p(out))
    return st, out


def call_kernel_grad_batched(c, kind, X, X2):
    out = c.buf(c.B, 1 + c.d)
    work = c.work(c.lib.gpn_grad_work_bytes(c.n, c.m, c.d, 0), c.B)
    st = c.lib.gpn_kernel_grad_batched(c.stream, kind, c.B, _p(X), 0, c.n, _p(X2), 0, c.m, c.d, _p(c.var), _p(c.ls), c.d, _p(c.G), c.m,
                                       c.n * c.m, _p(work), _p(out))
    return st, out


def call_kernel_grad_x2(c, kind, X, X2, b):
    out = c.buf(c.m, c.d)
    work = c.work(c.lib.gpn_grad_x2_work_bytes(c.n, c.m, c.d))
    st = c.lib.gpn_kernel_grad_x2(c.stream, kind, _p(X), c.n, _p(X2), c.m, c.d, _p(c.var[b:]), _p(c.ls[b]), c.d, _p(c.G[b]), c.m,
                                  c.inp.scale, 0, _p(work), _p(out))
    return st, out


def call_kernel_grad_x2_batched(c, kind, X, X2):
    out = c.buf(c.B, c.m, c.d)
    work = c.work(c.lib.gpn_grad_x2_work_bytes(c.n, c.m, c.d), c.B)
    st = c.lib.gpn_kernel_grad_x2_batched(c.stream, kind, c.B, _p(X), 0, c.n, _p(X2), 0, c.m, c.d, _p(c.var), _p(c.ls), c.d, _p(c.G), c.m,
                                          c.n * c.m, c.inp.scale, 0, _p(work), _p(out))
    return st, out


def call_lml_grad(c, kind, X, X2, b):
    out = c.buf(2 + c.d)
    work = c.work(c.lib.gpn_grad_work_bytes(c.n, c.n, c.d, 1))
    st = c.lib.gpn_lml_grad(c.stream, kind, _p(X), c.n, c.d, _p(c.var[b:]), _p(c.ls[b]), c.d, _p(c.Plow[b]), c.n, _p(c.at[b]), c.n, c.dy,
                            _p(work), _p(out))
    return st, out


def call_lml_grad_batched(c, kind, X, X2):
    out = c.buf(c.B, 2 + c.d)
    work = c.work(c.lib.gpn_grad_work_bytes(c.n, c.n, c.d, 1), c.B)
    st = c.lib.gpn_lml_grad_batched(c.stream, kind, c.B, _p(X), 0, c.n, c.d, _p(c.var), _p(c.ls), c.d, _p(c.Plow), c.n, c.n * c.n,
                                    _p(c.at), c.n, c.dy * c.n, c.dy, _p(work), _p(out))
    return st, out


def call_loo_grad(c, kind, X, X2, b):
    out = c.buf(2 + c.d)
    nbytes = int(c.lib.gpn_loo_grad_work_bytes(c.n, c.d))
    work = c.work(nbytes)
    st = c.lib.gpn_loo_grad(c.stream, kind, _p(X), c.n, c.d, _p(c.var[b:]), _p(c.ls[b]), c.d, _p(c.Plow[b]), c.n, _p(c.at[b]), c.n,
                            _p(c.wt[b]), c.n, c.dy, _p(work), nbytes, _p(out))
    return st, out


def call_loo_grad_batched(c, kind, X, X2):
    out = c.buf(c.B, 2 + c.d)
    nbytes = int(c.lib.gpn_loo_grad_batched_work_bytes(c.n, c.d, c.B))
    work = c.work(nbytes)
    st = c.lib.gpn_loo_grad_batched(c.stream, kind, c.B, _p(X), 0, c.n, c.d, _p(c.var), _p(c.ls), c.d, _p(c.Plow), c.n, c.n * c.n,
                                    _p(c.at), c.n, c.dy * c.n, _p(c.wt), c.n, c.dy * c.n, c.dy, _p(work), nbytes, _p(out))
    return st, out


SWEEPS = {"kernel_grad": (call_kernel_grad, call_kernel_grad_batched), "kernel_grad_x2": (call_kernel_grad_x2, call_kernel_grad_x2_batched),
          "lml_grad": (call_lml_grad, call_lml_grad_batched), "loo_grad": (call_loo_grad, call_loo_grad_batched)}


@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("family", list(SWEEPS))
def test_sweeps(ctx, family, kind):
    c = ctx
    single, batched = SWEEPS[family]
    ok = served("gpn_" + family, kind)
    assert ok == served("gpn_%s_batched" % family, kind)
    X, X2 = c.begin(ok)
    st, out = single(c, kind, X, X2, 1)
    stb, outb = batched(c, kind, X, X2)
    if not ok:
        return refused(c, max(st, stb))
    assert st == 0 and stb == 0
    check(family, kind, 1, {"out": out})
    for b in range(c.B):
        check(family, kind, b, {"out": outb[b]})
        assert torch.equal(outb[b], single(c, kind, X, X2, b)[1])


# ---- the whole-path entries -------------------------------------------------------------------------------------------------------------
def call_lml_forward(c, kind, X, b, saving=False):
    A, winv = c.buf(c.rows, c.lda, zero=True), c.buf(c.sW)
    info, out3 = c.buf(1, dtype=torch.int32), c.buf(3)
    args = (c.stream, kind, _p(X), c.n, c.d, _p(c.Y), None, c.dy, _p(c.var[b:]), _p(c.ls[b]), c.d, _p(c.noise[b:]), _p(A), c.lda, _p(winv),
            _p(info), _p(out3))
    if saving:
        Ksave = c.buf(c.n, c.lda)
        return c.lib.gpn_lml_forward_saving(*args, _p(Ksave)), A, info, out3, Ksave
    return c.lib.gpn_lml_forward(*args), A, info, out3, None


def call_lml_forward_batched(c, kind, X):
    A, winv = c.buf(c.B, c.rows, c.lda, zero=True), c.buf(c.B, c.sW)
    info, out3 = c.buf(c.B, dtype=torch.int32), c.buf(c.B, 3)
    st = c.lib.gpn_lml_forward_batched(c.stream, kind, c.B, _p(X), 0, c.n, c.d, _p(c.Y), 0, None, 0, c.dy, _p(c.var), _p(c.ls), c.d,
                                       _p(c.noise), _p(A), c.lda, c.sA, _p(winv), c.sW, _p(info), _p(out3))
    return st, A, info, out3


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_lml_forward(ctx, kind):
    c = ctx
    ok = served("gpn_lml_forward", kind)
    X, _ = c.begin(ok)
    st, A, info, out3, _ = call_lml_forward(c, kind, X, 1)
    sts, As, infos, out3s, Ksave = call_lml_forward(c, kind, X, 1, saving=True)
    stb, Ab, infob, out3b = call_lml_forward_batched(c, kind, X)
    # the ragged form takes more than 256 rows (test_ragged_forward_and_backward): here its kind check alone is reached
    n_of = torch.full((c.B,), c.n, dtype=torch.int32, device=c.dev)
    str_ = c.lib.gpn_lml_forward_ragged(c.stream, kind, c.B, _p(X), 0, c.n, _p(n_of), c.d, _p(c.Y), 0, c.dy, _p(c.var), _p(c.ls), c.d,
                                        _p(c.noise), _p(Ab), c.lda, c.sA, _p(c.buf(c.B, c.sW)), c.sW, _p(infob), _p(out3b))
    if not ok:
        refused(c, max(st, sts, stb))
        assert str_ == -2
        return
    assert st == 0 and sts == 0 and stb == 0 and str_ == -6
    assert int(info) == 0 and int(infos) == 0 and int(infob.abs().max()) == 0
    check("lml", kind, 1, {"out3": out3})
    assert torch.equal(out3s, out3) and torch.equal(As[:c.n + c.dy, :c.n].tril(), A[:c.n + c.dy, :c.n].tril())
    # the saved copy is K + noise I itself: that kind's entries (lower triangle)
    var, ls, noise = c.inp.hyp(1)
    Kyy = kr.kern(kr.KIND_NAMES[kind], c.inp.X, None, var, ls, xr.LD)[0] + xr.LD(noise) * np.eye(c.n, dtype=xr.LD)
    e64 = xr.abs_err(kr.kern(kr.KIND_NAMES[kind], c.inp.X, None, var, ls, np.float64)[0] + noise * np.eye(c.n), Kyy)
    low = np.tril(np.ones((c.n, c.n), dtype=bool))
    assert xr.abs_err(Ksave[:, :c.n].cpu().numpy()[low], Kyy[low]) <= xr.tol(e64, "K")
    for b in range(c.B):
        check("lml", kind, b, {"out3": out3b[b]})
        _, A1, _, o1, _ = call_lml_forward(c, kind, X, b)
        assert torch.equal(out3b[b], o1) and torch.equal(Ab[b, :c.n + c.dy, :c.n].tril(), A1[:c.n + c.dy, :c.n].tril())


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_lml_backward(ctx, kind):
    c = ctx
    ok = served("gpn_lml_backward", kind)
    fk = kind if ok else 0                      # a refused call still gets a valid factor (Rbf's): only its kind is wrong
    A, winv, _, _ = c.factor(fk, 1)
    Ab, winvb, _, _ = c.factor(fk)
    X, _ = c.begin(ok)
    lib = c.lib

    def single(b, A, winv):
        work = c.work(lib.gpn_lml_backward_work_bytes(c.n, c.dy, c.d))
        grads, resid = c.buf(2 + c.d), c.buf(c.n, c.dy)
        st = lib.gpn_lml_backward(c.stream, kind, _p(X), c.n, c.d, _p(c.var[b:]), _p(c.ls[b]), c.d, _p(A), c.lda, _p(winv), c.dy, _p(work),
                                  _p(grads), _p(resid))
        return st, grads, resid

    st, grads, resid = single(1, A[0], winv[0])
    workb = c.work(lib.gpn_lml_backward_batched_work_bytes(c.n, c.dy, c.d, c.B))
    gradsb, residb = c.buf(c.B, 2 + c.d), c.buf(c.B, c.n, c.dy)
    stb = lib.gpn_lml_backward_batched(c.stream, kind, c.B, _p(X), 0, c.n, c.d, _p(c.var), _p(c.ls), c.d, _p(Ab), c.lda, c.sA, _p(winvb), c.sW,
                                       c.dy, _p(workb), _p(gradsb), _p(residb))
    n_of = torch.full((c.B,), c.n, dtype=torch.int32, device=c.dev)
    str_ = lib.gpn_lml_backward_ragged(c.stream, kind, c.B, _p(X), 0, c.n, _p(n_of), c.d, _p(c.var), _p(c.ls), c.d, _p(Ab), c.lda, c.sA,
                                       _p(winvb), c.sW, c.dy, _p(workb), _p(gradsb))
    if not ok:
        refused(c, max(st, stb))
        assert str_ == -2
        return
    assert st == 0 and stb == 0 and str_ == -6          # (ragged: more than 256 rows; the kind check comes first)
    check("lml", kind, 1, {"grads": grads, "grad_resid": resid})
    for b in range(c.B):
        check("lml", kind, b, {"grads": gradsb[b], "grad_resid": residb[b]})
        _, g1, r1 = single(b, Ab[b], winvb[b])
        assert torch.equal(gradsb[b], g1) and torch.equal(residb[b], r1)


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_lml_refine_and_residual_part(ctx, kind):
    c = ctx
    ok = served("gpn_lml_refine", kind)
    assert ok == served("gpn_refine_resid_part", kind)
    b = 1
    A, winv, _, out3f = c.factor(kind if ok else 0, b)
    X, _ = c.begin(ok)
    lib = c.lib
    work = c.work(lib.gpn_lml_refine_work_bytes(c.n, c.dy))
    out3 = c.buf(3)
    if ok:
        out3.copy_(out3f[0])
    st = lib.gpn_lml_refine(c.stream, kind, _p(X), c.n, c.d, _p(c.Y), None, c.dy, _p(c.var[b:]), _p(c.ls[b]), c.d, _p(c.noise[b:]), _p(A), c.lda,
                            _p(winv), _p(work), _p(out3))
    ntri = int(lib.gpn_refine_tile_count(c.n))
    lds = (c.n + 127) // 128 * 128
    pwork = c.work(lib.gpn_refine_resid_part_work_bytes(c.dy, ntri))
    ka = c.buf(c.dy, lds, 2)
    a = torch.zeros(c.dy, lds, dtype=torch.float64, device=c.dev)               # vectors are [dy][round_up(n, 128)]
    a[:, :c.n] = c.at[b]
    stp = lib.gpn_refine_resid_part(c.stream, kind, _p(X), c.n, c.d, _p(c.var[b:]), _p(c.ls[b]), c.d, _p(c.noise[b:]), _p(a), c.dy, 0, ntri,
                                    _p(pwork), _p(ka))
    if not ok:
        return refused(c, max(st, stp))
    assert st == 0 and stp == 0
    check("lml", kind, b, {"out3": out3})
    assert torch.equal(out3[0], out3f[0, 0])                        # the log-determinant is kept
    kav = ka.cpu().numpy().astype(xr.LD)
    check("lml", kind, b, {"ka": torch.tensor(np.asarray(kav[:, :c.n, 0] + kav[:, :c.n, 1], dtype=np.float64))})


@pytest.mark.parametrize("full_cov", [0, 1])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_predict(ctx, kind, full_cov):
    c = ctx
    ok = served("gpn_predict", kind)
    assert ok == served("gpn_predict_blocked", kind)
    b = 1
    A, winv, _, _ = c.factor(kind if ok else 0, b)
    wb = torch.zeros(max(1, int(c.lib.gpn_block_inverse_bytes(c.n)) // 8), dtype=torch.float64, device=c.dev)
    assert c.lib.gpn_block_inverse(c.stream, _p(A), c.n, c.lda, _p(winv), _p(wb)) == 0
    X, X2 = c.begin(ok)
    lib = c.lib
    one = int(lib.gpn_predict_work_bytes(c.n, c.m, c.dy))
    outs = []
    for blocked in (False, True):
        work = c.work(2 * one if blocked else one)
        mean, var = c.buf(c.m, c.dy), c.buf(c.m, c.m) if full_cov else c.buf(c.m)
        head = (c.stream, kind, _p(X), c.n, c.d, _p(X2), c.m, None, _p(c.var[b:]), _p(c.ls[b]), c.d, _p(A), c.lda, _p(winv))
        tail = (c.dy, full_cov, _p(work), _p(mean), _p(var))
        st = lib.gpn_predict_blocked(*head, _p(wb), *tail) if blocked else lib.gpn_predict(*head, *tail)
        outs.append((st, mean, var))
    if not ok:
        return refused(c, max(o[0] for o in outs))
    for st, mean, var in outs:
        assert st == 0
        check("lml", kind, b, {"mean": mean, ("cov" if full_cov else "var"): var})


# ---- the Laplace / EP tile entries ---------------------------------------------------------------------------------------------------------
def call_laplace(c, kind, X, b):
    lib = c.lib
    sys_ = c.buf(c.n + 3, c.lda)
    st = [lib.gpn_laplace_system(c.stream, kind, _p(X), c.n, c.d, _p(c.var[b:]), _p(c.ls[b]), c.d, _p(c.s[b]), _p(sys_), c.lda)]
    rows = lib.gpn_laplace_rows_work_bytes(c.n)
    mv, dg, gr = c.buf(c.n), c.buf(c.n), c.buf(1 + c.d)
    st.append(lib.gpn_laplace_matvec(c.stream, kind, _p(X), c.n, c.d, _p(c.var[b:]), _p(c.ls[b]), c.d, _p(c.vec[b, 0]), _p(c.work(rows)), _p(mv)))
    st.append(lib.gpn_laplace_diag(c.stream, kind, _p(X), c.n, c.d, _p(c.var[b:]), _p(c.ls[b]), c.d, _p(c.s[b]), _p(c.Plow[b]), c.n,
                                   _p(c.work(rows)), _p(dg)))
    st.append(lib.gpn_laplace_grad(c.stream, kind, _p(X), c.n, c.d, _p(c.var[b:]), _p(c.ls[b]), c.d, _p(c.s[b]), _p(c.Plow[b]), c.n,
                                   _p(c.vec[b, 1]), _p(c.vec[b, 2]), _p(c.vec[b, 3]), _p(c.work(lib.gpn_laplace_grad_work_bytes(c.n, c.d))), _p(gr)))
    return st, {"system": sys_, "matvec": mv, "diag": dg, "grad": gr}


def call_laplace_batched(c, kind, X):
    lib = c.lib
    B, sv = c.B, 4 * c.n                          # the vectors of model b: vec[b, k], stride 4 n
    sys_ = c.buf(B, c.n + 3, c.lda)
    st = [lib.gpn_laplace_system_batched(c.stream, kind, B, _p(X), 0, c.n, c.d, _p(c.var), _p(c.ls), c.d, _p(c.s), c.n, _p(sys_), c.lda,
                                         (c.n + 3) * c.lda)]
    rows = lib.gpn_laplace_rows_work_bytes(c.n)
    mv, dg, gr = c.buf(B, c.n), c.buf(B, c.n), c.buf(B, 1 + c.d)
    st.append(lib.gpn_laplace_matvec_batched(c.stream, kind, B, _p(X), 0, c.n, c.d, _p(c.var), _p(c.ls), c.d, _p(c.vec[:, 0]), sv,
                                             _p(c.work(rows, B)), _p(mv)))
    st.append(lib.gpn_laplace_diag_batched(c.stream, kind, B, _p(X), 0, c.n, c.d, _p(c.var), _p(c.ls), c.d, _p(c.s), c.n, _p(c.Plow), c.n,
                                           c.n * c.n, _p(c.work(rows, B)), _p(dg)))
    # s, a, u, d1 share one stride: s rides in a copy laid out like the vectors
    sv4 = torch.stack([c.s, c.vec[:, 1], c.vec[:, 2], c.vec[:, 3]], 1).contiguous()
    st.append(lib.gpn_laplace_grad_batched(c.stream, kind, B, _p(X), 0, c.n, c.d, _p(c.var), _p(c.ls), c.d, _p(sv4[:, 0]), _p(c.Plow), c.n,
                                           c.n * c.n, _p(sv4[:, 1]), _p(sv4[:, 2]), _p(sv4[:, 3]), sv,
                                           _p(c.work(lib.gpn_laplace_grad_work_bytes(c.n, c.d), B)), _p(gr)))
    return st, {"system": sys_, "matvec": mv, "diag": dg, "grad": gr}


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_laplace_entries(ctx, kind):
    c = ctx
    names = ["gpn_laplace_%s%s" % (e, s) for e in ("system", "matvec", "diag", "grad") for s in ("", "_batched")]
    ok = served(names[0], kind)
    assert all(served(nm, kind) == ok for nm in names)
    X, _ = c.begin(ok)
    st, out = call_laplace(c, kind, X, 1)
    stb, outb = call_laplace_batched(c, kind, X)
    if not ok:
        assert all(s < 0 for s in st + stb), (st, stb)
        return c.assert_untouched()
    assert st == [0] * 4 and stb == [0] * 4

    def lower(sysbuf):                             # the entries the call writes; the rest keeps the buffer's fill
        assert bool((sysbuf[c.n:] == SENTINEL).all()) and bool((sysbuf[:c.n, c.n:] == SENTINEL).all())
        assert bool((sysbuf[:c.n, :c.n].triu(1) == torch.full_like(sysbuf[:c.n, :c.n], SENTINEL).triu(1)).all())
        return sysbuf[:c.n, :c.n].tril()

    def compare(b, o):
        want, tol, how = kr.reference("laplace", kind, b)["system"]
        err = kr.metric(lower(o["system"]).cpu().numpy(), np.tril(want), how)
        print("laplace %s b %d system: err %.2e tol %.1e (err / tol %.3f)" % (kr.KIND_NAMES[kind], b, err, tol, err / tol))
        assert err <= tol, ("system", kr.KIND_NAMES[kind], b, err, tol)
        check("laplace", kind, b, {k: v for k, v in o.items() if k != "system"})

    compare(1, out)
    for b in range(c.B):
        compare(b, {k: v[b] for k, v in outb.items()})
        _, o1 = call_laplace(c, kind, X, b)
        for k in o1:
            assert torch.equal(outb[k][b], o1[k]), (k, b)


# ---- the block-cyclic drivers on a 1 x 1 grid with a null communicator: status only ----------------------------------------------------------
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_dist_entries_status(ctx, kind):
    c = ctx
    lib = c.lib
    ok = served("gpn_dist_lml_forward", kind)
    b, tile = 1, 128
    X, X2 = c.begin(ok)
    hyp = (_p(c.var[b:]), _p(c.ls[b]), c.d, _p(c.noise[b:]))

    def aligned(nbytes):
        assert nbytes > 0
        t = c.buf(nbytes // 8 + 32)
        off = (-t.data_ptr() % 256) // 8
        return t[off:], nbytes

    w, wbytes = aligned(int(lib.gpn_dist_work_bytes(0, 1, 1, c.n, c.d, c.dy, tile)))
    out4 = c.buf(4)
    st = [lib.gpn_dist_lml_forward(c.stream, None, 0, 1, 1, kind, _p(X), c.n, c.d, _p(c.Y), c.dy, *hyp, tile, _p(w), wbytes, _p(out4))]
    rw, rbytes = aligned(int(lib.gpn_dist_lml_refine_work_bytes(0, 1, 1, c.n, c.d, c.dy, tile)))
    out4r = c.buf(4)
    if ok:
        out4r.copy_(out4)
    st.append(lib.gpn_dist_lml_refine(c.stream, None, 0, 1, 1, kind, _p(X), c.n, c.d, _p(c.Y), c.dy, *hyp, tile, _p(w), _p(rw), rbytes, _p(out4r)))
    gw, gbytes = aligned(int(lib.gpn_dist_grad_work_bytes(0, 1, 1, c.n, c.d, c.dy, tile)))
    out4g, grads, resid = c.buf(4), c.buf(2 + c.d), c.buf(c.n, c.dy)
    st.append(lib.gpn_dist_lml_grad(c.stream, None, 0, 1, 1, kind, _p(X), c.n, c.d, _p(c.Y), c.dy, *hyp, tile, _p(gw), gbytes, _p(out4g),
                                    _p(grads), _p(resid)))
    pw, pbytes = aligned(int(lib.gpn_dist_predict_work_bytes(0, 1, 1, c.n, c.d, c.dy, c.m, tile, 0)))
    out4p, mean, var = c.buf(4), c.buf(c.m, c.dy), c.buf(c.m)
    st.append(lib.gpn_dist_predict(c.stream, None, 0, 1, 1, kind, _p(X), c.n, c.d, _p(c.Y), c.dy, _p(X2), c.m, None, *hyp, tile, 0, _p(pw), pbytes,
                                   _p(out4p), _p(mean), _p(var)))
    torch.cuda.synchronize()
    if not ok:
        assert all(s < 0 for s in st), st
        return c.assert_untouched()
    assert st == [0] * 4, st


# ---- the ragged LML forms with a served kind: more than 256 rows, two models of different lengths ---------------------------------------
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_ragged_forward_and_backward(ctx, kind):
    """kr.RAGGED_N = 289 padded rows, models of 289 and 257 points (d = 1, dy = 2): out3 and the gradients of every model meet the
    long-double GP on its own points for THIS kind; a kind that is not served is refused with the buffers untouched."""
    c, lib = ctx, ctx.lib
    r = kr.ragged_inputs()
    B, n, d, dy = kr.RAGGED_BATCH, kr.RAGGED_N, kr.RAGGED_D, c.dy
    ok = served("gpn_lml_forward_ragged", kind)
    assert ok == served("gpn_lml_backward_ragged", kind)
    c.begin(ok)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=c.dev)
    X = t(r["X"]) if ok else torch.full((n, d), float("nan"), dtype=torch.float64, device=c.dev)
    Y, var, ls, noise = t(r["Y"]), t(r["var"]), t(r["ls"]), t(r["noise"])
    n_of = torch.tensor(kr.RAGGED_N_OF, dtype=torch.int32, device=c.dev)
    lda, rows = int(lib.gpn_factor_ld(n, dy)), int(lib.gpn_factor_rows(n, dy))
    sA, sW = rows * lda, int(lib.gpn_winv_bytes(n)) // 8
    A, winv = c.buf(B, rows, lda, zero=True), c.buf(B, sW)
    info, out3 = c.buf(B, dtype=torch.int32), c.buf(B, 3)
    st = lib.gpn_lml_forward_ragged(c.stream, kind, B, _p(X), 0, n, _p(n_of), d, _p(Y), 0, dy, _p(var), _p(ls), d, _p(noise), _p(A), lda, sA,
                                    _p(winv), sW, _p(info), _p(out3))
    work = c.work(lib.gpn_lml_backward_batched_work_bytes(n, dy, d, B))
    grads = c.buf(B, 2 + d)
    if ok:
        assert st == 0 and int(info.abs().max()) == 0
        Af, wf = A, winv
    else:                                        # the backward of a refused kind still gets a valid factor: Rbf's
        Af = torch.zeros(B, rows, lda, dtype=torch.float64, device=c.dev)
        wf = torch.zeros(B, sW, dtype=torch.float64, device=c.dev)
        i0, o0 = torch.zeros(B, dtype=torch.int32, device=c.dev), torch.zeros(B, 3, dtype=torch.float64, device=c.dev)
        assert lib.gpn_lml_forward_ragged(c.stream, 0, B, _p(t(r["X"])), 0, n, _p(n_of), d, _p(Y), 0, dy, _p(var), _p(ls), d, _p(noise), _p(Af),
                                          lda, sA, _p(wf), sW, _p(i0), _p(o0)) == 0
    stb = lib.gpn_lml_backward_ragged(c.stream, kind, B, _p(X), 0, n, _p(n_of), d, _p(var), _p(ls), d, _p(Af), lda, sA, _p(wf), sW, dy,
                                      _p(work), _p(grads))
    if not ok:
        return refused(c, max(st, stb))
    assert stb == 0
    for b in range(B):
        check("ragged", kind, b, {"out3": out3[b], "grads": grads[b]})
