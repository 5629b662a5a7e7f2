"""
Host-side orchestration over the C ABI (include/gpnative.h): turns torch CUDA
(HIP) tensors into device pointers + the current HIP stream, owns the factor
buffers, and exposes the differentiable log-marginal-likelihood.

Everything here requires fp64 tensors resident on a HIP device.  There is no
CPU code path: a CPU tensor raises `NativeError`.
"""
import ctypes
import math

import torch

from . import _native
from ._native import NativeError

KINDS = {"Rbf": 0, "Matern52": 1, "Matern32": 2, "Exp": 3, "Matern12": 3, "SqDist": 4, "Periodic": 5}
GPN_FULL, GPN_LOWER = 0, 1
LEAF = 128   # leaf block of the factorisation = padding granule of factor buffers (gpn_common.h)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _req(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise NativeError(
                "gptorch_amd runs on an AMD GPU only (no CPU fallback): got a tensor on %s; "
                "move the model/data with .cuda() first" % t.device)
        if t.dtype != torch.float64:
            raise TypeError("gptorch_amd computes in fp64 (gptorch TensorType); got %s" % t.dtype)


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def round_up(x, m):
    return (x + m - 1) // m * m


# ----------------------------------------------------------------------------
# K assembly
# ----------------------------------------------------------------------------
def kernel_matrix(kind, X, X2, variance, length_scales, noise=None, out=None, ldk=None, lower=False):
    """K(X, X2) as a new [n, m] tensor, or written into `out` (leading dim ldk)."""
    _req(X, X2, variance, length_scales, noise)
    X = _c(X.detach())
    n, d = X.shape
    if X2 is not None:
        X2 = _c(X2.detach())
        m = X2.shape[0]
        if X2.shape[1] != d:
            raise ValueError("X and X2 must have the same input dimension")
    else:
        m = n
    if out is None:
        out = torch.empty(n, m, dtype=torch.float64, device=X.device)
        ldk = m
    variance, length_scales = _c(variance.detach()), _c(length_scales.detach())
    noise = None if noise is None else _c(noise.detach())
    st = _native.lib().gpn_kernel_matrix(
        _stream(X.device), KINDS[kind], _ptr(X), n, _ptr(X2), m, d, _ptr(variance), _ptr(length_scales),
        length_scales.numel(), _ptr(noise), GPN_LOWER if lower else GPN_FULL, _ptr(out), ldk)
    _native.check(st, "gpn_kernel_matrix")
    return out


def zeros(rows, cols, device):
    """a zeroed [rows, cols] fp64 buffer: torch owns the memory, the library clears it (hipMemsetAsync on the current
    stream) -- the large factor / inverse buffers are not cleared by an elementwise torch kernel."""
    t = torch.empty(rows, cols, dtype=torch.float64, device=device)
    st = _native.lib().gpn_fill_zero(_stream(t.device), _ptr(t), t.numel() * 8)
    _native.check(st, "gpn_fill_zero")
    return t


# ----------------------------------------------------------------------------
# factor buffers + Cholesky
# ----------------------------------------------------------------------------
class Factor:
    """A factor buffer (see gpnative.h): n x n lower Cholesky factor in the
    top-left corner of `A` (rows x ld, zero padded), `e` extra rows holding
    (L^-1 R)^T, and the inverses of the 128x128 diagonal leaf blocks in `winv`."""

    def __init__(self, n, e, device):
        lib = _native.lib()
        self.n, self.e = int(n), int(e)
        self.ld = int(lib.gpn_factor_ld(n, e))
        self.rows = int(lib.gpn_factor_rows(n, e))
        self.A = zeros(self.rows, self.ld, device)
        self.winv = torch.empty(max(1, int(lib.gpn_winv_bytes(n)) // 8), dtype=torch.float64, device=device)
        self.info = torch.zeros(1, dtype=torch.int32, device=device)
        self.jitter_rung = -1
        self.generation = 0          # bumped by every factorisation into this buffer
        self._winv_full = None       # explicit L^-1 (lower_inverse), valid for one generation
        self._refine_work = None     # workspace of gpn_lml_refine (allocated on first use)
        self.refined = False

    @property
    def device(self):
        return self.A.device

    def extra(self):
        """[e, n] view: (L^-1 R)^T after factorisation."""
        return self.A[self.n:self.n + self.e, :self.n]

    def lower(self):
        """n x n copy of L with a zeroed upper triangle (torch.cholesky's output)."""
        out = torch.empty(self.n, self.n, dtype=torch.float64, device=self.device)
        if self.n:
            st = _native.lib().gpn_copy_matrix(_stream(self.device), _ptr(self.A), self.n, self.n, self.ld,
                                               _ptr(out), self.n, 1)
            _native.check(st, "gpn_copy_matrix")
        return out

    def pack_rhs(self, R, M=None):
        """extra rows <- (R - M)^T, R [n, e]."""
        _req(R, M)
        R = _c(R.detach())
        M = None if M is None else _c(M.detach())
        if self.e:
            self.A[self.n:self.n + self.e, self.n:].zero_()   # corner accumulates -alpha alpha^T
            st = _native.lib().gpn_pack_rhs(_stream(self.device), _ptr(R), _ptr(M), self.n, self.e,
                                            _ptr(self.A[self.n]), self.ld)
            _native.check(st, "gpn_pack_rhs")

    def potrf(self, check=True):
        """In-place factorisation; returns the LAPACK-style info (host int; syncs) or,
        with check=False, enqueues only and returns None (read self.info later)."""
        self.info.zero_()
        self.generation += 1
        self._winv_full = None
        st = _native.lib().gpn_potrf_lower(_stream(self.device), _ptr(self.A), self.n, self.e, self.ld,
                                           _ptr(self.winv), _ptr(self.info))
        _native.check(st, "gpn_potrf_lower")
        return int(self.info.item()) if check else None

    def lml_terms(self):
        """tensor [3]: sum log L_ii, ||extra||_F^2, LML (gpr.py:63-67)."""
        out = torch.empty(3, dtype=torch.float64, device=self.device)
        st = _native.lib().gpn_lml_reduce(_stream(self.device), _ptr(self.A), self.n, self.e, self.ld, _ptr(out))
        _native.check(st, "gpn_lml_reduce")
        return out

    def solve_right_lt(self, B, m):
        """B[m, :n] <- B * L^-T in place; B must be a [rows >= round_up(m,16), ld] buffer
        with ld == self.ld whose padding is zero."""
        st = _native.lib().gpn_trsm_right_lt(_stream(self.device), _ptr(self.A), self.n, self.ld, _ptr(self.winv),
                                             _ptr(B), m, B.stride(0))
        _native.check(st, "gpn_trsm_right_lt")
        return B


class FactorBatch:
    """`batch` factor buffers of one shape in ONE allocation (problem b at stride sA / sW), for
    gpn_lml_forward_batched / gpn_potrf_lower_batched; factor(b) is a Factor VIEW of problem b (same memory),
    usable with every single-model entry point afterwards (predict, backward ...)."""

    def __init__(self, batch, n, e, device):
        lib = _native.lib()
        self.batch, self.n, self.e = int(batch), int(n), int(e)
        self.ld = int(lib.gpn_factor_ld(n, e))
        self.rows = int(lib.gpn_factor_rows(n, e))
        self.sA = self.rows * self.ld
        self.sW = max(2, int(lib.gpn_winv_bytes(n)) // 8)
        self.A = zeros(self.batch * self.rows, self.ld, device)
        self.winv = torch.empty(self.batch * self.sW, dtype=torch.float64, device=device)
        self.info = torch.zeros(self.batch, dtype=torch.int32, device=device)
        self.out = torch.empty(self.batch, 3, dtype=torch.float64, device=device)
        self.generation = 0          # bumped by every lml_forward_batched into these buffers
        self._backward_work = None   # workspace of gpn_lml_backward_batched (allocated on first use, reused by a fit loop)

    def nbytes(self):
        w = 0 if self._backward_work is None else self._backward_work.numel()
        r = getattr(self, "_refine_work", None)
        w += 0 if r is None else r.numel()
        return 8 * (self.A.numel() + self.winv.numel() + w)

    def factor(self, b):
        f = Factor.__new__(Factor)
        f.n, f.e, f.ld, f.rows = self.n, self.e, self.ld, self.rows
        f.A = self.A[b * self.rows:(b + 1) * self.rows]
        f.winv = self.winv[b * self.sW:(b + 1) * self.sW]
        f.info = self.info[b:b + 1]
        f.jitter_rung = -1
        f.generation = 0
        f._winv_full = None
        f._refine_work = None
        f.refined = False
        return f


def lml_forward_batched(kind, X, R, variance, length_scales, noise, fb=None, refine=False, n_of=None):
    """GPR.log_likelihood (gpr.py:47-67) of `batch` models in lock step (gpn_lml_forward_batched): X [n, d] shared or
    [batch, n, d]; R = Y - m(X) [n, dy] shared or [batch, n, dy]; variance [batch], length_scales [batch, nls],
    noise [batch].  -> (FactorBatch, terms [batch, 3]); NO host synchronisation: the caller reads fb.info and
    replays the models whose info != 0 through the sequential path (jitter ladder).
    refine: follow the lock-step factorisation with gpn_lml_refine on every model's factor (what lml_forward does from
    refine_min_n() rows on: the same call on the same factor, so the refined terms are bit-identical too).
    n_of (int32 device tensor [batch]): a RAGGED batch (gpn_lml_forward_ragged) -- model b has n_of[b] <= n points, X [batch, n, d] and
    R [batch, n, dy] are padded to n rows (the padding is not read into any result); no refinement."""
    _req(X, R, variance, length_scales, noise)
    batch = int(variance.numel())
    shared_x, shared_r = X.dim() == 2, R.dim() == 2
    n, d = X.shape[-2], X.shape[-1]
    e = R.shape[-1]
    if R.shape[-2] != n:
        raise ValueError("X and Y must have same # data.")
    if fb is None or fb.batch != batch or fb.n != n or fb.e != e or fb.A.device != X.device:
        fb = FactorBatch(batch, n, e, X.device)
    Xc, Rc = _c(X.detach()), _c(R.detach())
    var, ls, nz = _c(variance.detach().reshape(batch)), _c(length_scales.detach().reshape(batch, -1)), _c(noise.detach().reshape(batch))
    fb.generation += 1
    if n_of is not None:
        if shared_x or shared_r or refine:
            raise ValueError("ragged batches hold every model's own (padded) data and are not refined")
        st = _native.lib().gpn_lml_forward_ragged(
            _stream(X.device), KINDS[kind], batch, _ptr(Xc), n * d, n, _ptr(n_of), d, _ptr(Rc), n * e, e, _ptr(var), _ptr(ls), ls.shape[1],
            _ptr(nz), _ptr(fb.A), fb.ld, fb.sA, _ptr(fb.winv), fb.sW, _ptr(fb.info), _ptr(fb.out))
        _native.check(st, "gpn_lml_forward_ragged")
        return fb, fb.out
    st = _native.lib().gpn_lml_forward_batched(
        _stream(X.device), KINDS[kind], batch, _ptr(Xc), 0 if shared_x else n * d, n, d, _ptr(Rc), 0 if shared_r else n * e,
        None, 0, e, _ptr(var), _ptr(ls), ls.shape[1], _ptr(nz), _ptr(fb.A), fb.ld, fb.sA, _ptr(fb.winv), fb.sW,
        _ptr(fb.info), _ptr(fb.out))
    _native.check(st, "gpn_lml_forward_batched")
    if refine and n > 0:
        lib = _native.lib()
        if getattr(fb, "_refine_work", None) is None:
            fb._refine_work = torch.empty(max(1, int(lib.gpn_lml_refine_work_bytes(n, e)) // 8), dtype=torch.float64, device=X.device)
        for b in range(batch):                       # (3 % of an evaluation each; enqueued before anybody reads `info`)
            Xb = Xc if shared_x else Xc[b]
            Rb = Rc if shared_r else Rc[b]
            st = lib.gpn_lml_refine(_stream(X.device), KINDS[kind], _ptr(Xb), n, d, _ptr(Rb), None, e, _ptr(var[b:b + 1]), _ptr(ls[b]), ls.shape[1],
                                    _ptr(nz[b:b + 1]), _ptr(fb.A[b * fb.rows:]), fb.ld, _ptr(fb.winv[b * fb.sW:]), _ptr(fb._refine_work),
                                    _ptr(fb.out[b]))
            _native.check(st, "gpn_lml_refine")
    return fb, fb.out


def lml_backward_batched(kind, X, variance, length_scales, fb, need_resid=False, n_of=None):
    """the closed-form backward of the `batch` models of an lml_forward_batched call in lock step (gpn_lml_backward_batched):
    -> (grads [batch, 2 + nls] = dLML/d(variance, length_scales, noise) per model w.r.t. the CONSTRAINED values,
        dLML/dR [batch, n, dy] or None).  Per model bit-identical to _backward.lml_backward on that model's factor."""
    _req(X, variance, length_scales)
    batch, n, dy = fb.batch, fb.n, fb.e
    ls = _c(length_scales.detach().reshape(batch, -1))
    nls = ls.shape[1]
    lib = _native.lib()
    need = max(1, int(lib.gpn_lml_backward_batched_work_bytes(n, dy, nls, batch)) // 8)
    if fb._backward_work is None or fb._backward_work.numel() < need:
        fb._backward_work = torch.empty(need, dtype=torch.float64, device=fb.A.device)
    out = torch.empty(batch, 2 + nls, dtype=torch.float64, device=fb.A.device)
    g_R = torch.empty(batch, n, dy, dtype=torch.float64, device=fb.A.device) if need_resid else None
    Xc = _c(X.detach())
    if n_of is not None:                              # the backward of a ragged batch (gpn_lml_backward_ragged): no dLML/dR
        if need_resid or Xc.dim() != 3:
            raise ValueError("ragged batches: every model's own padded points, zero mean functions")
        st = lib.gpn_lml_backward_ragged(_stream(fb.A.device), KINDS[kind], batch, _ptr(Xc), n * Xc.shape[-1], n, _ptr(n_of), Xc.shape[-1],
                                         _ptr(_c(variance.detach().reshape(batch))), _ptr(ls), nls, _ptr(fb.A), fb.ld, fb.sA,
                                         _ptr(fb.winv), fb.sW, dy, _ptr(fb._backward_work), _ptr(out))
        _native.check(st, "gpn_lml_backward_ragged")
        return out, None
    st = lib.gpn_lml_backward_batched(_stream(fb.A.device), KINDS[kind], batch, _ptr(Xc), 0 if Xc.dim() == 2 else n * Xc.shape[-1], n,
                                      Xc.shape[-1], _ptr(_c(variance.detach().reshape(batch))), _ptr(ls), nls, _ptr(fb.A), fb.ld, fb.sA,
                                      _ptr(fb.winv), fb.sW, dy, _ptr(fb._backward_work), _ptr(out), _ptr(g_R))
    _native.check(st, "gpn_lml_backward_batched")
    return out, g_R


REFINE_MIN_N = 12288
JITTER_TRIES = 10  # functions.py:21 max_tries


# ---- evaluations without a host read-back (hipGraph capture of an optimiser step: models/base.py _optimize_captured) --------
# While a DeferredInfo is active, lml_forward enqueues ONE attempt (no jitter), leaves the factorisation's `info` word on the
# device and ORs "info != 0" into the holder's flag instead of reading it back: nothing in the evaluation synchronises the host,
# so evaluation + closed-form backward + optimiser step capture into one graph.  The caller looks at the flag every so many
# replays and repeats a chunk that saw a failure through the ordinary path (jitter ladder of functions.py:20-43).
_DEFERRED = []


class DeferredInfo:
    def __init__(self, device):
        self.flag = torch.zeros(1, dtype=torch.int32, device=device)

    def __enter__(self):
        _DEFERRED.append(self)
        return self

    def __exit__(self, *exc):
        _DEFERRED.pop()
        return False

    def note(self, info):
        torch.maximum(self.flag, (info != 0).to(torch.int32), out=self.flag)


def _ladder(attempt, tries=None):
    """functions.py:20-43: plain try, then +10^(-max_tries+i) I for i = 0..max_tries-1 (max_tries = 10 by default), then
    RuntimeError("Max tries exceeded.").  `attempt(jitter)` -> info."""
    tries = JITTER_TRIES if tries is None else int(tries)
    def run(jitter):
        info = attempt(jitter)
        if info < 0:
            # GPN_INFO_INTERNAL: a hand-over inside the leaf kernel failed -- says nothing about the
            # matrix, so adding jitter would only hide it
            raise NativeError("factorisation reported the internal status %d (not a property of the matrix)" % info)
        return info

    if run(None) == 0:
        return -1
    for i in range(tries):
        if run(10.0 ** (-tries + i)) == 0:
            return i
    raise RuntimeError("Max tries exceeded.")


def cholesky_factor(x, rhs=None):
    """functions.cholesky (functions.py:46-47) of a dense SPD matrix `x` [n, n];
    optional rhs [n, k] is forward-substituted on the way (extra rows)."""
    _req(x, rhs)
    if x.dim() != 2 or x.shape[0] != x.shape[1]:
        raise RuntimeError("cholesky: expected a square matrix")
    n = x.shape[0]
    e = 0 if rhs is None else rhs.shape[1]
    f = Factor(n, e, x.device)
    xs = _c(x.detach())

    def attempt(jitter):
        if n:
            st = _native.lib().gpn_copy_matrix(_stream(x.device), _ptr(xs), n, n, n, _ptr(f.A), f.ld, 1)
            _native.check(st, "gpn_copy_matrix")
            if jitter is not None:
                f.A.diagonal()[:n].add_(jitter)
        if e:
            f.pack_rhs(rhs)
        return f.potrf()

    f.jitter_rung = _ladder(attempt)
    return f


def kernel_factor_async(kind, X, variance, length_scales, noise, R=None, factor=None):
    """kernel_factor without the host read-back of `info`: everything is enqueued on the
    current stream and the caller inspects f.info afterwards (a non-zero info must be
    replayed through kernel_factor for the jitter ladder).  Lets several independent
    models (hyper-parameter restarts) be in flight on different HIP streams."""
    _req(X, variance, length_scales, noise, R)
    n = X.shape[0]
    e = 0 if R is None else R.shape[1]
    f = factor if (factor is not None and factor.n == n and factor.e == e and factor.device == X.device) \
        else Factor(n, e, X.device)
    kernel_matrix(kind, X, None, variance, length_scales, noise=noise, out=f.A, ldk=f.ld, lower=True)
    if e:
        f.pack_rhs(R)
    f.potrf(check=False)
    f.jitter_rung = -1
    return f


def kernel_factor(kind, X, variance, length_scales, noise, R=None, factor=None):
    """Fused K(X)+noise*I assembly -> Cholesky (+ forward substitution of R).
    gpr.py:61-62 / 104-106.  Reuses `factor` (same n, e) when given."""
    _req(X, variance, length_scales, noise, R)
    n = X.shape[0]
    e = 0 if R is None else R.shape[1]
    f = factor if (factor is not None and factor.n == n and factor.e == e and factor.device == X.device) \
        else Factor(n, e, X.device)

    def attempt(jitter):
        if jitter is None:
            nz = noise
        elif noise is None:
            nz = torch.full((1,), jitter, dtype=torch.float64, device=X.device)
        else:
            nz = noise + jitter
        kernel_matrix(kind, X, None, variance, length_scales, noise=nz, out=f.A, ldk=f.ld, lower=True)
        if e:
            f.pack_rhs(R)
        return f.potrf()

    f.jitter_rung = _ladder(attempt)
    return f


def refine_min_n(expression=False, grid=False):
    """from this many rows on, lml_forward follows the factorisation with one refinement step of the quadratic form
    (gpn_lml_refine).  The plain value's distance to the exact one grows like N^1.85 (5.8e-10 at N = 8192, 7.6e-9 at
    32768, measured) and north_star's tolerance is 1e-8 ABSOLUTE against a reference that is itself 3.4e-9 off at
    32768: below about 10^4 rows the step buys nothing, above it costs about 3 %.  GPN_REFINE_MIN_N overrides
    (0 = never) and is taken VERBATIM for every caller: the 1/2 and 2/3 factors below scale the built-in default only.
    expression=True: covariance expressions (Linear / Constant terms grow the top eigenvalue like N |x|^2, so the
    quadratic form's sensitivity to the factor's rounding is an order of magnitude above a stationary kernel's: the
    reference's example model at N = 8192 sits 2e-8 from its golden unrefined, whichever leaf kernel factors it) refine
    from half that size on.
    grid=True: the block-cyclic drivers (their tile-wide trailing updates accumulate over K = 1024..2048 per launch, a
    different rounding profile from the single-GPU panels: C2's matrix on a 1 x 1 grid of 2048-wide tiles sits 0.9-1.1e-8
    from the golden unrefined) refine from two thirds of that size on (8192 rows)."""
    import os
    env = os.environ.get("GPN_REFINE_MIN_N")
    if env is not None:
        v = int(env)
    elif expression:
        v = REFINE_MIN_N // 2
    elif grid:
        v = (2 * REFINE_MIN_N) // 3
    else:
        v = REFINE_MIN_N
    return v if v > 0 else 1 << 62


def lml_forward(kind, X, R, variance, length_scales, noise, factor=None, refine=None):
    """GPR.log_likelihood (gpr.py:47-67) as ONE library call (gpn_lml_forward: assembly ->
    factorisation with the residual riding along -> reductions) plus the jitter ladder of
    functions.py:20-43 on its info word.  -> (Factor, terms [3]: sum log L_ii, |alpha|^2, LML).
    refine (default: N >= refine_min_n()): follow it with gpn_lml_refine, after which terms[1] is
    y^T Kyy^-1 y corrected to second order in the factor's rounding error (and terms[2] the LML with it).
    GPN_REFINE_SAVED_K=1 (opt-in): the assembly also keeps a pristine copy of Kyy (gpn_lml_forward_saving: n * ld * 8 more
    bytes) that the refinement's residual pass reads back instead of re-computing every entry -- the same refined value bit
    for bit; C3: refinement 3.3 -> 2.1 ms, assembly 1.8 -> 2.6 ms (twice the writes), evaluation 183.3 -> 182.8 ms.  Off by
    default: 0.25 % for 8.6 GB."""
    _req(X, R, variance, length_scales, noise)
    n, e = R.shape
    if X.shape[0] != n:
        raise ValueError("X and Y must have same # data.")
    f = factor if (factor is not None and factor.n == n and factor.e == e and factor.device == X.device) \
        else Factor(n, e, X.device)
    Xc, Rc = _c(X.detach()), _c(R.detach())
    var, ls, nz0 = _c(variance.detach()), _c(length_scales.detach()), _c(noise.detach())
    out = torch.empty(3, dtype=torch.float64, device=X.device)
    lib = _native.lib()

    def attempt(jitter):
        nz = nz0 if jitter is None else nz0 + jitter
        f.generation += 1
        f._winv_full = None
        if do_refine and f._refine_work is None:
            f._refine_work = torch.empty(max(1, int(lib.gpn_lml_refine_work_bytes(n, e)) // 8), dtype=torch.float64, device=X.device)
        if do_refine and save_k:
            # the assembly also leaves a pristine copy of Kyy's lower triangle (the factorisation overwrites it in place): the
            # refinement's residual pass READS it instead of re-computing every kernel entry
            if getattr(f, "_ksave", None) is None:
                f._ksave = torch.empty(n, f.ld, dtype=torch.float64, device=X.device)
            st = lib.gpn_lml_forward_saving(_stream(X.device), KINDS[kind], _ptr(Xc), n, Xc.shape[1], _ptr(Rc), None, e,
                                            _ptr(var), _ptr(ls), ls.numel(), _ptr(nz), _ptr(f.A), f.ld, _ptr(f.winv),
                                            _ptr(f.info), _ptr(out), _ptr(f._ksave))
            _native.check(st, "gpn_lml_forward_saving")
            st = lib.gpn_lml_refine_dense(_stream(X.device), _ptr(f._ksave), f.ld, 0.0, n, _ptr(Rc), None, e, _ptr(f.A), f.ld,
                                          _ptr(f.winv), _ptr(f._refine_work), _ptr(out))
            _native.check(st, "gpn_lml_refine_dense")
            return int(f.info.item())
        st = lib.gpn_lml_forward(_stream(X.device), KINDS[kind], _ptr(Xc), n, Xc.shape[1], _ptr(Rc), None, e,
                                 _ptr(var), _ptr(ls), ls.numel(), _ptr(nz), _ptr(f.A), f.ld, _ptr(f.winv),
                                 _ptr(f.info), _ptr(out))
        _native.check(st, "gpn_lml_forward")
        if do_refine:
            # enqueued before the info word is read back (no idle GPU during the host round trip); if the
            # factorisation failed its result is discarded with the attempt
            st = lib.gpn_lml_refine(_stream(X.device), KINDS[kind], _ptr(Xc), n, Xc.shape[1], _ptr(Rc), None, e,
                                    _ptr(var), _ptr(ls), ls.numel(), _ptr(nz), _ptr(f.A), f.ld, _ptr(f.winv),
                                    _ptr(f._refine_work), _ptr(out))
            _native.check(st, "gpn_lml_refine")
        return int(f.info.item())

    do_refine = (n >= refine_min_n()) if refine is None else bool(refine)
    import os
    save_k = os.environ.get("GPN_REFINE_SAVED_K", "0") == "1"
    if _DEFERRED:
        # one attempt, no read-back (see DeferredInfo): the caller inspects the flag later
        save_k = False
        _no_sync = _DEFERRED[-1]
        f.generation += 1
        f._winv_full = None
        if do_refine and f._refine_work is None:
            f._refine_work = torch.empty(max(1, int(lib.gpn_lml_refine_work_bytes(n, e)) // 8), dtype=torch.float64, device=X.device)
        st = lib.gpn_lml_forward(_stream(X.device), KINDS[kind], _ptr(Xc), n, Xc.shape[1], _ptr(Rc), None, e,
                                 _ptr(var), _ptr(ls), ls.numel(), _ptr(nz0), _ptr(f.A), f.ld, _ptr(f.winv),
                                 _ptr(f.info), _ptr(out))
        _native.check(st, "gpn_lml_forward")
        if do_refine:
            st = lib.gpn_lml_refine(_stream(X.device), KINDS[kind], _ptr(Xc), n, Xc.shape[1], _ptr(Rc), None, e,
                                    _ptr(var), _ptr(ls), ls.numel(), _ptr(nz0), _ptr(f.A), f.ld, _ptr(f.winv),
                                    _ptr(f._refine_work), _ptr(out))
            _native.check(st, "gpn_lml_refine")
        _no_sync.note(f.info)
        f.jitter_rung = -1
        f.refined = do_refine
        return f, out
    f.jitter_rung = _ladder(attempt)
    f.refined = do_refine
    return f, out


TRI_A_UPPER, TRI_A_LOWER, TRI_B_UPPER, TRI_B_LOWER = 1, 2, 4, 8


def gemm_nt(A, B, M, N, K, alpha=1.0, beta=0.0, C=None, lower=False, tri=0):
    """C[M,N] = alpha*A[M,K]*B[N,K]^T + beta*C (row strides taken from the tensors)."""
    _req(A, B, C)
    if C is None:
        C = torch.empty(M, N, dtype=torch.float64, device=A.device)
    st = _native.lib().gpn_gemm_nt(_stream(A.device), M, N, K, alpha, _ptr(A), A.stride(0), _ptr(B), B.stride(0),
                                   beta, _ptr(C), C.stride(0), int(lower), tri)       # lower: False/True or 2 = trapezoid
    _native.check(st, "gpn_gemm_nt")
    return C


def gemm_nt_stair(A, B, C, M, nblocks, blk, K, step, diag, alpha=-1.0, beta=1.0):
    """staircase contraction (gpnative.h gpn_gemm_nt_stair): C[M, nblocks*blk] = alpha A B^T + beta C where column
    block b only has the rows from b*step on and, with diag, a lower-only first square."""
    _req(A, B, C)
    st = _native.lib().gpn_gemm_nt_stair(_stream(A.device), M, nblocks, blk, K, alpha, _ptr(A), A.stride(0), _ptr(B), B.stride(0),
                                         beta, _ptr(C), C.stride(0), step, 1 if diag else 0)
    _native.check(st, "gpn_gemm_nt_stair")
    return C


def matmul_nt(A, B, alpha=1.0):
    """alpha * A @ B^T for arbitrary 2-D fp64 device tensors through the native contraction (pads K to
    a multiple of 16 and re-packs operands that are not 16-byte aligned row-major); for the
    autograd nodes of the off-hot-path `functions` / `util` surface."""
    _req(A, B)
    M, K = A.shape
    N = B.shape[0]
    if B.shape[1] != K:
        raise RuntimeError("matmul_nt: inner dimensions differ")
    out = torch.zeros(M, N, dtype=torch.float64, device=A.device)
    if M == 0 or N == 0 or K == 0:
        return out
    Kp = round_up(K, 16)

    def prep(T, rows):
        T = T.detach()
        ok = T.stride(1) == 1 and T.stride(0) % 2 == 0 and T.stride(0) >= Kp and T.data_ptr() % 16 == 0 \
            and K == Kp and T.shape[0] % 16 == 0
        if ok:
            return T
        P = torch.zeros(round_up(rows, 16), Kp, dtype=torch.float64, device=T.device)
        P[:rows, :K] = T
        return P
    return gemm_nt(prep(A, M), prep(B, N), M, N, Kp, alpha=alpha, C=out)


def gemm_nt_batched(A, B, M, N, K, batch, sA, sB, C, alpha=1.0, beta=0.0, lower=False, tri=0):
    """`batch` contractions of one shape in one launch: C[z] = alpha*A_z*B_z^T + beta*C[z], A_z = A + z*sA
    elements (row stride from the tensor), C [batch, rows, ld] contiguous."""
    _req(A, B, C)
    st = _native.lib().gpn_gemm_nt_batched(_stream(A.device), M, N, K, alpha, _ptr(A), A.stride(0), sA, _ptr(B), B.stride(0), sB,
                                           beta, _ptr(C), C.stride(1), C.stride(0), 1 if lower else 0, tri, batch)
    _native.check(st, "gpn_gemm_nt_batched")
    return C


def gemm_nt_batched_scaled(A, B, M, N, K, batch, sA, sB, C, alphas, beta=0.0, lower=False, tri=0):
    """gemm_nt_batched with one scale per problem from device memory: C[z] = alphas[z]*A_z*B_z^T + beta*C[z] (alphas: `batch`
    contiguous fp64 on the operands' device), per problem bit-identical to gemm_nt(alpha=alphas[z])."""
    _req(A, B, C, alphas)
    if alphas.numel() < batch or not alphas.is_contiguous():
        raise RuntimeError("gemm_nt_batched_scaled: alphas must hold `batch` contiguous values")
    st = _native.lib().gpn_gemm_nt_batched_scaled(_stream(A.device), M, N, K, _ptr(alphas), _ptr(A), A.stride(0), sA, _ptr(B), B.stride(0), sB,
                                                  beta, _ptr(C), C.stride(1), C.stride(0), 1 if lower else 0, tri, batch)
    _native.check(st, "gpn_gemm_nt_batched_scaled")
    return C


def transpose(src):
    _req(src)
    src = _c(src.detach())
    rows, cols = src.shape
    dst = torch.empty(cols, rows, dtype=torch.float64, device=src.device)
    st = _native.lib().gpn_transpose(_stream(src.device), _ptr(src), rows, cols, cols, _ptr(dst), rows)
    _native.check(st, "gpn_transpose")
    return dst


def row_sumsq(A, rows, cols):
    out = torch.empty(rows, dtype=torch.float64, device=A.device)
    st = _native.lib().gpn_row_sumsq(_stream(A.device), _ptr(A), rows, cols, A.stride(0), _ptr(out))
    _native.check(st, "gpn_row_sumsq")
    return out


def dot2d_raw(x, ldx, sx, y, ldy, sy, rows, cols, batch, device):
    """out[z] = <x_z, y_z> over a rows x cols view (gpn_dot2d_batched; x, y: pointers, y None: the plain sum) -> [batch]."""
    out = torch.empty(batch, dtype=torch.float64, device=device)
    st = _native.lib().gpn_dot2d_batched(_stream(device), x, ldx, sx, y, ldy, sy, rows, cols, _ptr(out), batch)
    _native.check(st, "gpn_dot2d_batched")
    return out


def dot2d(x, y=None):
    """sum(x * y) (y None: sum(x)) of 2-D fp64 device tensors with unit inner stride, as a 0-dim tensor: ONE launch with a fixed
    summation order (the scalar sums of the sparse bound, sparse_gpr.py:139-151; their lock-step form is the same kernel)."""
    _req(x, y)
    x = x if x.stride(1) == 1 else x.contiguous()
    if y is not None:
        y = y if y.stride(1) == 1 else y.contiguous()
    return dot2d_raw(_ptr(x), x.stride(0), 0, _ptr(y), 0 if y is None else y.stride(0), 0, x.shape[0], x.shape[1], 1, x.device)[0]


def diag_sum(A, m):
    """sum of the first m diagonal entries of a row-major matrix (0-dim tensor; see dot2d)."""
    _req(A)
    return dot2d_raw(_ptr(A), A.stride(0) + 1, 0, None, 0, 0, m, 1, 1, A.device)[0]


def lik_expect(kind, params, f_mean, f_var, y, nodes, weights, want_value=True, want_mean=True, want_var=True, want_params=True):
    """gpn_lik_expect: the Gauss-Hermite expectation of a non-Gaussian log-likelihood under N(f_mean[:, k], f_var) summed over
    the entries, with its gradients -> (value 0-dim, g_mean [rows, dy], g_var [rows], g_params [2]); an output that is not
    wanted is None.  params: a [2] device tensor (Student-t: df, scale^2) or None; nodes / weights: [H] device tensors of
    the rule (None for the Poisson closed form).  ONE call, no host synchronisation."""
    _req(params, f_mean, f_var, y, nodes, weights)
    if f_mean.dim() != 2 or tuple(y.shape) != tuple(f_mean.shape) or f_var.shape != (f_mean.shape[0],):
        raise ValueError("expect f_mean [rows, dy], y [rows, dy] and f_var [rows]; got %s, %s, %s"
                         % (tuple(f_mean.shape), tuple(y.shape), tuple(f_var.shape)))
    f_mean = f_mean if f_mean.stride(1) == 1 else f_mean.contiguous()
    y = y if y.stride(1) == 1 else y.contiguous()
    f_var = _c(f_var)
    rows, dy = f_mean.shape
    dev = f_mean.device
    work = torch.empty(2 * ((rows + _native.LIK_ROWS_PER_GROUP - 1) // _native.LIK_ROWS_PER_GROUP), dtype=torch.float64, device=dev)
    value = torch.empty((), dtype=torch.float64, device=dev) if want_value else None
    g_mean = torch.empty(rows, dy, dtype=torch.float64, device=dev) if want_mean else None
    g_var = torch.empty(rows, dtype=torch.float64, device=dev) if want_var else None
    g_params = torch.empty(2, dtype=torch.float64, device=dev) if want_params else None
    st = _native.lib().gpn_lik_expect(_stream(dev), kind, _ptr(params), _ptr(f_mean), f_mean.stride(0), _ptr(f_var), _ptr(y), y.stride(0),
                                      rows, dy, _ptr(nodes), _ptr(weights), 0 if nodes is None else nodes.numel(), _ptr(work),
                                      work.numel() * 8, _ptr(value), _ptr(g_mean), dy, _ptr(g_var), _ptr(g_params))
    _native.check(st, "gpn_lik_expect")
    return value, g_mean, g_var, g_params


def _robustmax_operands(f_mean, f_var, nodes, weights):
    if f_mean.dim() != 2 or f_mean.shape[1] < 2 or f_var.shape != (f_mean.shape[0],):
        raise ValueError("expect f_mean [rows, C >= 2] and f_var [rows]; got %s, %s" % (tuple(f_mean.shape), tuple(f_var.shape)))
    if nodes.shape != weights.shape or nodes.dim() != 1:
        raise ValueError("expect nodes [H] and weights [H]; got %s, %s" % (tuple(nodes.shape), tuple(weights.shape)))
    return (f_mean if f_mean.stride(1) == 1 else f_mean.contiguous()), _c(f_var), _c(nodes), _c(weights)


def lik_expect_robustmax(f_mean, f_var, labels, eps, nodes, weights, want_value=True, want_mean=True, want_var=True):
    """gpn_lik_expect_robustmax: the expected log-likelihood of the robust-max multi-class likelihood under N(f_mean[:, c], f_var)
    (one variance per row) summed over the rows, with its gradients -> (value 0-dim, g_mean [rows, C], g_var [rows]); an output
    that is not wanted is None.  labels [rows]: doubles holding the class indices.  ONE call, no host synchronisation."""
    _req(f_mean, f_var, labels, nodes, weights)
    f_mean, f_var, nodes, weights = _robustmax_operands(f_mean, f_var, nodes, weights)
    rows, C = f_mean.shape
    if labels.shape != (rows,):
        raise ValueError("expect labels [%d]; got %s" % (rows, tuple(labels.shape)))
    labels = _c(labels)
    dev = f_mean.device
    g = _native.ROBUSTMAX_ROWS_PER_GROUP
    work = torch.empty((rows + g - 1) // g, dtype=torch.float64, device=dev)
    value = torch.empty((), dtype=torch.float64, device=dev) if want_value else None
    g_mean = torch.empty(rows, C, dtype=torch.float64, device=dev) if want_mean else None
    g_var = torch.empty(rows, dtype=torch.float64, device=dev) if want_var else None
    st = _native.lib().gpn_lik_expect_robustmax(_stream(dev), _ptr(f_mean), f_mean.stride(0), _ptr(f_var), _ptr(labels), rows, C, float(eps),
                                                _ptr(nodes), _ptr(weights), nodes.numel(), _ptr(work), work.numel() * 8, _ptr(value),
                                                _ptr(g_mean), C, _ptr(g_var))
    _native.check(st, "gpn_lik_expect_robustmax")
    return value, g_mean, g_var


def lik_robustmax_probs(f_mean, f_var, eps, nodes, weights):
    """gpn_lik_robustmax_probs -> p(y = c) [rows, C] of the robust-max likelihood under N(f_mean[:, c], f_var)."""
    _req(f_mean, f_var, nodes, weights)
    f_mean, f_var, nodes, weights = _robustmax_operands(f_mean, f_var, nodes, weights)
    rows, C = f_mean.shape
    probs = torch.empty(rows, C, dtype=torch.float64, device=f_mean.device)
    st = _native.lib().gpn_lik_robustmax_probs(_stream(f_mean.device), _ptr(f_mean), f_mean.stride(0), _ptr(f_var), rows, C, float(eps),
                                               _ptr(nodes), _ptr(weights), nodes.numel(), _ptr(probs), C)
    _native.check(st, "gpn_lik_robustmax_probs")
    return probs


# ----------------------------------------------------------------------------
# LaplaceGP (models/laplace.py): csrc/laplace.hip + the back-substitution of csrc/refine.hip
# ----------------------------------------------------------------------------
def _vec(t, n, what):
    _req(t)
    if t.numel() != n:
        raise ValueError("%s must have %d entries; got %s" % (what, n, tuple(t.shape)))
    return _c(t.detach().reshape(-1))


def _kargs(X, variance, length_scales):
    _req(X, variance, length_scales)
    Xc, var, ls = _c(X.detach()), _c(variance.detach()), _c(length_scales.detach())
    return Xc, var, ls, (_ptr(Xc), Xc.shape[0], Xc.shape[1], _ptr(var), _ptr(ls), ls.numel())


def lik_derivs(kind, f, y, want_value=True, want_d1=True, want_w=True, want_d3=True):
    """gpn_lik_derivs: sum log p(y_i | f_i) and, per point, d1 = dlp/df, W = -d2lp/df2, d3 = d3lp/df3 ->
    (value 0-dim, d1 [n], W [n], d3 [n]); an output that is not wanted is None.  No host synchronisation."""
    n = f.numel()
    f, y = _vec(f, n, "f"), _vec(y, n, "y")
    dev = f.device
    lib = _native.lib()
    work = torch.empty(max(1, int(lib.gpn_lik_derivs_work_bytes(n)) // 8), dtype=torch.float64, device=dev)
    outs = [torch.empty((), dtype=torch.float64, device=dev) if want_value else None]
    outs += [torch.empty(n, dtype=torch.float64, device=dev) if want else None for want in (want_d1, want_w, want_d3)]
    st = lib.gpn_lik_derivs(_stream(dev), kind, _ptr(f), _ptr(y), n, _ptr(work), work.numel() * 8, *[_ptr(o) for o in outs])
    _native.check(st, "gpn_lik_derivs")
    return tuple(outs)


def laplace_system(kind, X, variance, length_scales, s, out, ldo):
    """gpn_laplace_system: B = I + diag(s) K(X) diag(s), the entries on and below the diagonal, into `out` (leading dimension
    ldo; a factor buffer)."""
    Xc, var, ls, args = _kargs(X, variance, length_scales)
    s = _vec(s, Xc.shape[0], "s")
    _req(out)
    st = _native.lib().gpn_laplace_system(_stream(Xc.device), KINDS[kind], *args, _ptr(s), _ptr(out), ldo)
    _native.check(st, "gpn_laplace_system")
    return out


def _rows_work(n, device, work, batch=1):
    need = max(1, batch * int(_native.lib().gpn_laplace_rows_work_bytes(n)) // 8)      # (= gpn_laplace_rows_batched_work_bytes(n, batch))
    return work if (work is not None and work.numel() >= need and work.device == device) else torch.empty(need, dtype=torch.float64, device=device)


def laplace_matvec(kind, X, variance, length_scales, v, work=None):
    """gpn_laplace_matvec: K(X) v [n], matrix-free (work: a buffer of an earlier call to reuse)."""
    Xc, var, ls, args = _kargs(X, variance, length_scales)
    n = Xc.shape[0]
    v = _vec(v, n, "v")
    work = _rows_work(n, Xc.device, work)
    out = torch.empty(n, dtype=torch.float64, device=Xc.device)
    st = _native.lib().gpn_laplace_matvec(_stream(Xc.device), KINDS[kind], *args, _ptr(v), _ptr(work), _ptr(out))
    _native.check(st, "gpn_laplace_matvec")
    return out


def laplace_diag(kind, X, variance, length_scales, s, Binv, work=None):
    """gpn_laplace_diag: diag((K^-1 + W)^-1) [n] = (1 / s_i) sum_j K_ij s_j Binv_ji, Binv (row-major, lower triangle read)."""
    Xc, var, ls, args = _kargs(X, variance, length_scales)
    n = Xc.shape[0]
    s = _vec(s, n, "s")
    _req(Binv)
    work = _rows_work(n, Xc.device, work)
    out = torch.empty(n, dtype=torch.float64, device=Xc.device)
    st = _native.lib().gpn_laplace_diag(_stream(Xc.device), KINDS[kind], *args, _ptr(s), _ptr(Binv), Binv.stride(0), _ptr(work), _ptr(out))
    _native.check(st, "gpn_laplace_diag")
    return out


def laplace_grad(kind, X, variance, length_scales, s, Binv, a, u, d1):
    """gpn_laplace_grad: sum_ij G_ij dK_ij/d(variance, length_scales) [1 + nls] (CONSTRAINED values) with
    G = 1/2 a a^T - 1/2 diag(s) Binv diag(s) + 1/2 (u d1^T + d1 u^T)."""
    Xc, var, ls, args = _kargs(X, variance, length_scales)
    n = Xc.shape[0]
    s, a, u, d1 = _vec(s, n, "s"), _vec(a, n, "a"), _vec(u, n, "u"), _vec(d1, n, "d1")
    _req(Binv)
    lib = _native.lib()
    work = torch.empty(max(1, int(lib.gpn_laplace_grad_work_bytes(n, ls.numel())) // 8), dtype=torch.float64, device=Xc.device)
    out = torch.empty(1 + ls.numel(), dtype=torch.float64, device=Xc.device)
    st = lib.gpn_laplace_grad(_stream(Xc.device), KINDS[kind], *args, _ptr(s), _ptr(Binv), Binv.stride(0), _ptr(a), _ptr(u), _ptr(d1),
                              _ptr(work), _ptr(out))
    _native.check(st, "gpn_laplace_grad")
    return out


def backsub(f):
    """gpn_backsub: (L^-T alpha)^T [e, n] for the alpha^T in the extra rows of a factorised buffer."""
    lib = _native.lib()
    work = torch.empty(max(1, int(lib.gpn_backsub_work_bytes(f.n, f.e)) // 8), dtype=torch.float64, device=f.device)
    out = torch.empty(f.e, f.n, dtype=torch.float64, device=f.device)
    st = lib.gpn_backsub(_stream(f.device), _ptr(f.A), f.ld, _ptr(f.winv), f.n, f.e, _ptr(work), _ptr(out), f.n)
    _native.check(st, "gpn_backsub")
    return out


EP_STATS = ("sum_log_z", "site_evidence", "max_dtau", "max_dnu", "max_tau", "max_nu")      # gpn_ep_sites' statistics vector


def ep_sites(kind, y, m, mu, sigma2, tau, nu, damping, nodes=None, weights=None, moments_only=False, want_moments=True):
    """gpn_ep_sites: cavity, tilted moments, damped site update and statistics of one EP sweep ->
    (tau_new [n], nu_new [n], log Z^ [n], mu_hat [n], s2_hat [n], stats [6] as EP_STATS).  moments_only: no update, tau_new / nu_new
    are None; want_moments=False: the three per-point moments are None.  m: the prior mean at the points or None (zero);
    nodes / weights: the Gauss-Hermite rule of the logit link (None for probit).  No host synchronisation."""
    n = y.numel()
    y, mu, sigma2, tau, nu = (_vec(t, n, what) for t, what in ((y, "y"), (mu, "mu"), (sigma2, "sigma2"), (tau, "tau"), (nu, "nu")))
    m = None if m is None else _vec(m, n, "m")
    _req(nodes, weights)
    dev = y.device
    lib = _native.lib()

    def new(want, k=n):
        return torch.empty(k, dtype=torch.float64, device=dev) if want else None

    work = new(True, max(1, int(lib.gpn_ep_sites_work_bytes(n)) // 8))
    tau_new, nu_new = new(not moments_only), new(not moments_only)
    lz, mu_hat, s2_hat = new(want_moments), new(want_moments), new(want_moments)
    stats = new(True, len(EP_STATS))
    st = lib.gpn_ep_sites(_stream(dev), kind, n, _ptr(y), _ptr(m), _ptr(mu), _ptr(sigma2), _ptr(tau), _ptr(nu), float(damping), _ptr(nodes),
                          _ptr(weights), 0 if nodes is None else nodes.numel(), int(bool(moments_only)), _ptr(work), work.numel() * 8,
                          _ptr(tau_new), _ptr(nu_new), _ptr(lz), _ptr(mu_hat), _ptr(s2_hat), _ptr(stats))
    _native.check(st, "gpn_ep_sites")
    return tau_new, nu_new, lz, mu_hat, s2_hat, stats


# ---- the same in lock step (models/_laplace_lockstep.py): `batch` equal-shape models per launch.  X [n, d] shared or [batch, n, d],
# variance [batch], length_scales [batch, nls], vectors stacked [batch, n]; every row of every result is bit-identical to the
# single wrapper called on that model.  No host synchronisation.
def _kargs_batched(X, variance, length_scales):
    _req(X, variance, length_scales)
    batch = int(variance.numel())
    Xc, var, ls = _c(X.detach()), _c(variance.detach().reshape(batch)), _c(length_scales.detach().reshape(batch, -1))
    n, d = Xc.shape[-2], Xc.shape[-1]
    if Xc.dim() == 3 and Xc.shape[0] != batch:
        raise ValueError("stacked points must be [batch, n, d] with batch = %d; got %s" % (batch, tuple(Xc.shape)))
    return Xc, var, ls, batch, n, (batch, _ptr(Xc), 0 if Xc.dim() == 2 else n * d, n, d, _ptr(var), _ptr(ls), ls.shape[1])


def _rows(t, batch, n, what):
    _req(t)
    if tuple(t.shape) != (batch, n):
        raise ValueError("%s must be [%d, %d]; got %s" % (what, batch, n, tuple(t.shape)))
    return _c(t.detach())


def lik_derivs_batched(kind, f, y, want_value=True, want_d1=True, want_w=True, want_d3=True):
    """gpn_lik_derivs_batched: lik_derivs for f [batch, n] and y [n] (shared) or [batch, n] -> (value [batch], d1, W, d3
    [batch, n]); an output that is not wanted is None."""
    batch, n = f.shape
    f = _rows(f, batch, n, "f")
    y = _vec(y, n, "y") if y.dim() == 1 else _rows(y, batch, n, "y")
    dev = f.device
    lib = _native.lib()
    work = torch.empty(max(1, int(lib.gpn_lik_derivs_batched_work_bytes(n, batch)) // 8), dtype=torch.float64, device=dev)
    outs = [torch.empty(batch, dtype=torch.float64, device=dev) if want_value else None]
    outs += [torch.empty(batch, n, dtype=torch.float64, device=dev) if want else None for want in (want_d1, want_w, want_d3)]
    st = lib.gpn_lik_derivs_batched(_stream(dev), kind, batch, _ptr(f), n, _ptr(y), 0 if y.dim() == 1 else n, n, _ptr(work), work.numel() * 8,
                                    *[_ptr(o) for o in outs])
    _native.check(st, "gpn_lik_derivs_batched")
    return tuple(outs)


def laplace_system_batched(kind, X, variance, length_scales, s, fb):
    """gpn_laplace_system_batched: B_b = I + diag(s_b) K_b diag(s_b), on and below the diagonal, into the first `batch` slots of the
    FactorBatch fb (batch = variance.numel() <= fb.batch)."""
    Xc, var, ls, batch, n, args = _kargs_batched(X, variance, length_scales)
    s = _rows(s, batch, n, "s")
    if batch > fb.batch or n != fb.n:
        raise ValueError("%d systems of %d rows do not fit a FactorBatch of %d x %d" % (batch, n, fb.batch, fb.n))
    st = _native.lib().gpn_laplace_system_batched(_stream(Xc.device), KINDS[kind], *args, _ptr(s), n, _ptr(fb.A), fb.ld, fb.sA)
    _native.check(st, "gpn_laplace_system_batched")
    return fb


def laplace_matvec_batched(kind, X, variance, length_scales, v, work=None):
    """gpn_laplace_matvec_batched: K_b v_b [batch, n], matrix-free."""
    Xc, var, ls, batch, n, args = _kargs_batched(X, variance, length_scales)
    v = _rows(v, batch, n, "v")
    work = _rows_work(n, Xc.device, work, batch)
    out = torch.empty(batch, n, dtype=torch.float64, device=Xc.device)
    st = _native.lib().gpn_laplace_matvec_batched(_stream(Xc.device), KINDS[kind], *args, _ptr(v), n, _ptr(work), _ptr(out))
    _native.check(st, "gpn_laplace_matvec_batched")
    return out


def laplace_diag_batched(kind, X, variance, length_scales, s, Binv, ldb, sB, work=None):
    """gpn_laplace_diag_batched: diag((K_b^-1 + W_b)^-1) [batch, n]; Binv: a tensor (or device address) whose model b starts sB
    doubles after model 0, leading dimension ldb, lower triangle read."""
    Xc, var, ls, batch, n, args = _kargs_batched(X, variance, length_scales)
    s = _rows(s, batch, n, "s")
    work = _rows_work(n, Xc.device, work, batch)
    out = torch.empty(batch, n, dtype=torch.float64, device=Xc.device)
    st = _native.lib().gpn_laplace_diag_batched(_stream(Xc.device), KINDS[kind], *args, _ptr(s), n, _addr(Binv), ldb, sB, _ptr(work), _ptr(out))
    _native.check(st, "gpn_laplace_diag_batched")
    return out


def laplace_grad_batched(kind, X, variance, length_scales, s, Binv, ldb, sB, a, u, d1):
    """gpn_laplace_grad_batched: [batch, 1 + nls], row b = laplace_grad of model b (Binv as in laplace_diag_batched)."""
    Xc, var, ls, batch, n, args = _kargs_batched(X, variance, length_scales)
    s, a, u, d1 = _rows(s, batch, n, "s"), _rows(a, batch, n, "a"), _rows(u, batch, n, "u"), _rows(d1, batch, n, "d1")
    lib = _native.lib()
    nls = ls.shape[1]
    work = torch.empty(max(1, int(lib.gpn_laplace_grad_batched_work_bytes(n, nls, batch)) // 8), dtype=torch.float64, device=Xc.device)
    out = torch.empty(batch, 1 + nls, dtype=torch.float64, device=Xc.device)
    st = lib.gpn_laplace_grad_batched(_stream(Xc.device), KINDS[kind], *args, _ptr(s), _addr(Binv), ldb, sB, _ptr(a), _ptr(u), _ptr(d1), n,
                                      _ptr(work), _ptr(out))
    _native.check(st, "gpn_laplace_grad_batched")
    return out


def ep_sites_batched(kind, y, m, mu, sigma2, tau, nu, dampings, nodes=None, weights=None, moments_only=False, want_moments=True):
    """gpn_ep_sites_batched: ep_sites for mu, sigma2, tau, nu [batch, n], y [n] (shared) or [batch, n], m [batch, n] or None and
    dampings [batch] (a DEVICE tensor: every model its own) -> (tau_new, nu_new, log Z^, mu_hat, s2_hat [batch, n], stats [batch, 6]);
    an output that is not wanted is None."""
    batch, n = mu.shape
    mu, sigma2, tau, nu = (_rows(t, batch, n, what) for t, what in ((mu, "mu"), (sigma2, "sigma2"), (tau, "tau"), (nu, "nu")))
    y = _vec(y, n, "y") if y.dim() == 1 else _rows(y, batch, n, "y")
    m = None if m is None else _rows(m, batch, n, "m")
    dampings = _vec(dampings, batch, "dampings")
    _req(nodes, weights)
    dev = mu.device
    lib = _native.lib()

    def new(want, *shape):
        return torch.empty(*shape, dtype=torch.float64, device=dev) if want else None

    work = new(True, max(1, int(lib.gpn_ep_sites_batched_work_bytes(n, batch)) // 8))
    tau_new, nu_new = new(not moments_only, batch, n), new(not moments_only, batch, n)
    lz, mu_hat, s2_hat = new(want_moments, batch, n), new(want_moments, batch, n), new(want_moments, batch, n)
    stats = new(True, batch, len(EP_STATS))
    st = lib.gpn_ep_sites_batched(_stream(dev), kind, batch, n, _ptr(y), 0 if y.dim() == 1 else n, _ptr(m), _ptr(mu), _ptr(sigma2), _ptr(tau),
                                  _ptr(nu), _ptr(dampings), _ptr(nodes), _ptr(weights), 0 if nodes is None else nodes.numel(),
                                  int(bool(moments_only)), _ptr(work), work.numel() * 8, _ptr(tau_new), _ptr(nu_new), _ptr(lz), _ptr(mu_hat),
                                  _ptr(s2_hat), _ptr(stats))
    _native.check(st, "gpn_ep_sites_batched")
    return tau_new, nu_new, lz, mu_hat, s2_hat, stats


def _addr(t):
    return ctypes.c_void_p(t) if isinstance(t, int) else _ptr(t)


def backsub_batched(fb, batch=None):
    """gpn_backsub_batched: (L_b^-T alpha_b)^T [batch, e, n] for the extra rows of the first `batch` (default: all) factorised
    slots of a FactorBatch."""
    batch = fb.batch if batch is None else int(batch)
    lib = _native.lib()
    dev = fb.A.device
    work = torch.empty(max(1, int(lib.gpn_backsub_batched_work_bytes(fb.n, fb.e, batch)) // 8), dtype=torch.float64, device=dev)
    out = torch.empty(batch, fb.e, fb.n, dtype=torch.float64, device=dev)
    st = lib.gpn_backsub_batched(_stream(dev), batch, _ptr(fb.A), fb.ld, fb.sA, _ptr(fb.winv), fb.sW, fb.n, fb.e, _ptr(work), _ptr(out),
                                 fb.n, fb.e * fb.n)
    _native.check(st, "gpn_backsub_batched")
    return out


def padded_like_factor(f, m):
    """zeroed [round_up(m,128), f.ld] buffer for right-hand sides of solve_right_lt."""
    return zeros(round_up(max(m, 1), LEAF), f.ld, f.device)


def trtrs_lower(b, f):
    """functions.trtrs(b, L, lower=True) (functions.py:71-76): X = L^-1 b, b [n, k]."""
    _req(b)
    n, k = b.shape
    if n != f.n:
        raise RuntimeError("trtrs: size mismatch")
    Bt = padded_like_factor(f, k)
    if n and k:
        bs = _c(b.detach())
        st = _native.lib().gpn_transpose(_stream(b.device), _ptr(bs), n, k, k, _ptr(Bt), f.ld)
        _native.check(st, "gpn_transpose")
        f.solve_right_lt(Bt, k)
    out = torch.empty(n, k, dtype=torch.float64, device=b.device)
    if n and k:
        st = _native.lib().gpn_transpose(_stream(b.device), _ptr(Bt), k, n, f.ld, _ptr(out), k)
        _native.check(st, "gpn_transpose")
    return out


# ----------------------------------------------------------------------------
# GPR predictive equations (gpr.py:88-117) in transposed storage
# ----------------------------------------------------------------------------
def lower_inverse(f):
    """W = L^-1 (lower, row-major, zero padded [rows, ld]) of a factor, cached on it: with W every
    right-solve X L^T = B is ONE K-clipped contraction X = B W^T instead of a chain of ~2 n/128
    small launches -- worth its n^3/3 flops for a model that serves many predictions."""
    W = f._winv_full
    if W is None:
        from . import _backward
        U = _backward._upper_inverse(f)
        W = zeros(U.shape[0], U.shape[1], U.device)
        if f.n:
            st = _native.lib().gpn_transpose(_stream(f.device), _ptr(U), f.n, f.n, f.ld, _ptr(W), f.ld)
            _native.check(st, "gpn_transpose")
        f._winv_full = W
    return W


BLOCKED_PREDICT_MIN_N = 4096      # from here on a repeated prediction pays for the inverted 1024 x 1024 diagonal blocks


def block_inverses(f):
    """inverses of the 1024 x 1024 diagonal blocks of a factor (gpn_block_inverse), cached on it for one generation."""
    wb = getattr(f, "_wblock", None)
    if wb is None or wb[0] != f.generation:
        lib = _native.lib()
        buf = torch.empty(max(1, int(lib.gpn_block_inverse_bytes(f.n)) // 8), dtype=torch.float64, device=f.device)
        _native.check(lib.gpn_block_inverse(_stream(f.device), _ptr(f.A), f.n, f.ld, _ptr(f.winv), _ptr(buf)), "gpn_block_inverse")
        f._wblock = wb = (f.generation, buf)
    return wb[1]


def gpr_predict(kind, X, x_new, variance, length_scales, f, diag=True, use_inverse=False, mean_new=None, blocked=False):
    """Returns (m(x*) + A^T V  [n*, dy],  var) with A = L^-1 K(X, x*), V = L^-1 (Y - m) held
    in f.extra(); var = rowsumsq-reduced diag [n*] or full K(x*) - A^T A [n*, n*].  mean_new [n*, dy]: the mean
    function at the test points (gpr.py:107-108), None = zero.  blocked: the right-solve through the inverted 1024 x 1024
    diagonal blocks (built on first use, cached on the factor)."""
    ns = x_new.shape[0]
    n, dy = f.n, f.e
    if blocked and not use_inverse and dy > 0 and n >= BLOCKED_PREDICT_MIN_N:
        _req(X, x_new, variance, length_scales)
        lib = _native.lib()
        wb = block_inverses(f)
        Xc, Xs = _c(X.detach()), _c(x_new.detach())
        var, ls = _c(variance.detach()), _c(length_scales.detach())
        work = torch.empty(max(1, 2 * int(lib.gpn_predict_work_bytes(n, ns, dy)) // 8), dtype=torch.float64, device=f.device)
        mean = torch.empty(ns, dy, dtype=torch.float64, device=f.device)
        out = torch.empty((ns,) if diag else (ns, ns), dtype=torch.float64, device=f.device)
        ms = None if mean_new is None else _c(mean_new.detach().expand(ns, dy))
        st = lib.gpn_predict_blocked(_stream(f.device), KINDS[kind], _ptr(Xc), n, Xc.shape[1], _ptr(Xs), ns, _ptr(ms), _ptr(var), _ptr(ls),
                                     ls.numel(), _ptr(f.A), f.ld, _ptr(f.winv), _ptr(wb), dy, 0 if diag else 1, _ptr(work), _ptr(mean),
                                     _ptr(out))
        _native.check(st, "gpn_predict_blocked")
        return mean, out
    if not use_inverse and dy > 0:
        # one library call: K(x*, X) -> right-solve chain -> mean / variance (gpn_predict)
        _req(X, x_new, variance, length_scales)
        lib = _native.lib()
        Xc, Xs = _c(X.detach()), _c(x_new.detach())
        var, ls = _c(variance.detach()), _c(length_scales.detach())
        work = torch.empty(max(1, int(lib.gpn_predict_work_bytes(n, ns, dy)) // 8), dtype=torch.float64, device=f.device)
        mean = torch.empty(ns, dy, dtype=torch.float64, device=f.device)
        out = torch.empty((ns,) if diag else (ns, ns), dtype=torch.float64, device=f.device)
        ms = None if mean_new is None else _c(mean_new.detach().expand(ns, dy))
        st = lib.gpn_predict(_stream(f.device), KINDS[kind], _ptr(Xc), n, Xc.shape[1], _ptr(Xs), ns, _ptr(ms), _ptr(var), _ptr(ls),
                             ls.numel(), _ptr(f.A), f.ld, _ptr(f.winv), dy, 0 if diag else 1, _ptr(work), _ptr(mean), _ptr(out))
        _native.check(st, "gpn_predict")
        return mean, out
    Bt = padded_like_factor(f, ns)
    if use_inverse:
        Ks = padded_like_factor(f, ns)
        kernel_matrix(kind, x_new, X, variance, length_scales, out=Ks, ldk=f.ld)
        gemm_nt(Ks, lower_inverse(f), ns, n, round_up(n, 16), C=Bt, tri=TRI_B_LOWER)   # A^T = K(x*,X) W^T
    else:
        kernel_matrix(kind, x_new, X, variance, length_scales, out=Bt, ldk=f.ld)   # K(x*, X) = k_ys^T
        f.solve_right_lt(Bt, ns)                                                   # A^T = K(x*,X) L^-T
    kpad = round_up(n, 16)
    mean = gemm_nt(Bt, f.A[n:], ns, dy, kpad)                                  # A^T V
    if mean_new is not None:
        mean = mean + mean_new
    if diag:
        var = variance.detach().expand(ns) - row_sumsq(Bt, ns, n)              # Kdiag - colsumsq(A)
    else:
        var = kernel_matrix(kind, x_new, None, variance, length_scales)
        gemm_nt(Bt, Bt, ns, ns, kpad, alpha=-1.0, beta=1.0, C=var)
    return mean, var


# ----------------------------------------------------------------------------
# differentiable LML
# ----------------------------------------------------------------------------
class GPRLogLik(torch.autograd.Function):
    """log p(y | X, theta) of gpr.py:47-67 as one autograd node over the native
    pipeline  K assembly -> Cholesky (+ fused forward substitution) -> reductions.
    Inputs are the CONSTRAINED hyper-parameters (1-element / [D] device tensors)
    and the residual R = y - mean(x); output has shape (1,) like the reference."""

    @staticmethod
    def forward(ctx, X, R, variance, length_scales, noise, kind, holder):
        f, terms = lml_forward(kind, X, R, variance, length_scales, noise, factor=holder.get("factor"))
        holder["factor"] = f
        ctx.kind = kind
        ctx.factor = f
        ctx.generation = f.generation
        ctx.save_for_backward(X, R, variance, length_scales, noise)
        return terms[2:3].clone()

    @staticmethod
    def backward(ctx, grad_out):
        from . import _backward
        X, R, variance, length_scales, noise = ctx.saved_tensors
        f = ctx.factor
        if f.generation != ctx.generation:
            # the model's reusable buffer was refactorised by a later forward (two losses alive at
            # once): this node's factor is gone, rebuild it privately rather than differentiate
            # the wrong one
            f = kernel_factor(ctx.kind, X, variance, length_scales, noise, R=R)
        g_var, g_ls, g_noise, g_R = _backward.lml_backward(ctx.kind, X, variance, length_scales, noise, f)
        go = grad_out.reshape(())
        return (None, go * g_R if ctx.needs_input_grad[1] else None, go * g_var, go * g_ls, go * g_noise, None, None)


class BatchedGPRLogLik(torch.autograd.Function):
    """GPRLogLik for `batch` independent models of one shape in LOCK STEP (hyper-parameter restarts; the reference runs
    loss(); backward(); step() one model at a time, gptorch/models/base.py:260-269): X [n, d] shared or [batch, n, d],
    R = Y - m(X) [n, dy] shared or [batch, n, dy], variance [batch], length_scales [batch, nls], noise [batch] (CONSTRAINED
    values) -> LML [batch].  Forward = gpn_lml_forward_batched, backward = gpn_lml_backward_batched; a model whose
    factorisation reports info != 0 is replayed ALONE through lml_forward (jitter ladder of functions.py:20-43) into a
    private factor, and its backward runs on that factor.  Values and gradients are bit-identical, model by model, to
    GPRLogLik -- also from refine_min_n() rows on, where every model's quadratic form is refined as GPRLogLik's is."""

    @staticmethod
    def forward(ctx, X, R, variance, length_scales, noise, kind, holder, n_of=None):
        # n_of (int32 device tensor [batch]; `sizes` = the same numbers on the host in holder["sizes"]): a RAGGED group -- X, R padded
        # to the largest model (lml_forward_batched(n_of=...)): no refinement, no gradient w.r.t. R
        batch = int(variance.numel())
        sizes = holder.get("sizes") if n_of is not None else None
        fb, terms = lml_forward_batched(kind, X, R, variance, length_scales, noise, fb=holder.get("fb"),
                                        refine=n_of is None and X.shape[-2] >= refine_min_n(), n_of=n_of)
        holder["fb"] = fb
        out = terms[:, 2].clone()
        replayed = {}
        if _DEFERRED:
            # under hipGraph capture (multi_start_optimize(capture=True)): nothing may read `info` back -- it is OR-ed into the
            # capture's device flag, and a chunk of replays that saw a failure is repeated eagerly (through the ladder below)
            _DEFERRED[-1].note(fb.info.abs().max().reshape(1))
            info = None
        else:
            info = fb.info.cpu()                     # ONE read-back for the batch (the reference: one per model and step)
        for b in (torch.nonzero(info).reshape(-1).tolist() if (info is not None and bool(info.any())) else ()):
            if int(info[b]) != 0:
                nb = X.shape[-2] if sizes is None else sizes[b]
                f, t = lml_forward(kind, (X if X.dim() == 2 else X[b])[:nb], (R if R.dim() == 2 else R[b])[:nb], variance.reshape(batch)[b:b + 1],
                                   length_scales.reshape(batch, -1)[b], noise.reshape(batch)[b:b + 1])
                out[b] = t[2]
                replayed[b] = f
        ctx.kind, ctx.fb, ctx.generation, ctx.replayed = kind, fb, fb.generation, replayed
        ctx.n_of, ctx.sizes = n_of, sizes
        ctx.save_for_backward(X, R, variance, length_scales, noise)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from . import _backward
        X, R, variance, length_scales, noise = ctx.saved_tensors
        batch = int(variance.numel())
        fb = ctx.fb
        if fb.generation != ctx.generation:
            # the shared buffers were refactorised by a later forward: rebuild this node's factors privately
            fb, _ = lml_forward_batched(ctx.kind, X, R, variance, length_scales, noise, n_of=ctx.n_of)
        need_r = ctx.needs_input_grad[1]
        grads, g_R = lml_backward_batched(ctx.kind, X, variance, length_scales, fb, need_resid=need_r, n_of=ctx.n_of)
        nls = grads.shape[1] - 2
        for b, f in ctx.replayed.items():
            nb = X.shape[-2] if ctx.sizes is None else ctx.sizes[b]
            gv, gl, gn, gr = _backward.lml_backward(ctx.kind, (X if X.dim() == 2 else X[b])[:nb], variance.reshape(batch)[b:b + 1],
                                                    length_scales.reshape(batch, -1)[b], noise.reshape(batch)[b:b + 1], f)
            grads[b, 0:1], grads[b, 1:1 + nls], grads[b, 1 + nls:] = gv, gl, gn
            if need_r:
                g_R[b] = gr
        go = grad_out.reshape(batch)
        g_resid = None
        if need_r:
            g_resid = go[:, None, None] * g_R
            if R.dim() == 2:
                g_resid = g_resid.sum(0)
        return (None, g_resid, (go * grads[:, 0]).reshape(variance.shape), (go[:, None] * grads[:, 1:1 + nls]).reshape(length_scales.shape),
                (go * grads[:, 1 + nls]).reshape(noise.shape), None, None, None)


class DenseLogLik(torch.autograd.Function):
    """The same LML for a kernel matrix that arrives as a dense tensor (Sum / Product /
    Linear / White ... kernels, whose K(X) is composed by autograd from several assemblies):
    Kyy = K + noise I is copied into the factor buffer, the factorisation and the closed-form
    backward are the native ones, and dLML/dK = 1/2 (a a^T - dy Kyy^-1) is handed back to
    autograd as a dense [n, n] gradient for the kernels' own backward sweeps."""

    @staticmethod
    def forward(ctx, K, R, noise):
        n = K.shape[0]
        Kyy = K.detach().clone()
        Kyy.diagonal().add_(noise.detach()[0])
        f = cholesky_factor(Kyy, rhs=R)
        ctx.factor = f
        terms = f.lml_terms()
        f.refined = False
        if n >= refine_min_n():
            # the refinement step of the quadratic form; the residual pass reads the dense Kyy it was factorised from
            lib = _native.lib()
            e = R.shape[1]
            jitter = 0.0 if f.jitter_rung < 0 else 10.0 ** (-JITTER_TRIES + f.jitter_rung)
            work = torch.empty(max(1, int(lib.gpn_lml_refine_work_bytes(n, e)) // 8), dtype=torch.float64, device=K.device)
            Rc = _c(R.detach())
            st = lib.gpn_lml_refine_dense(_stream(K.device), _ptr(Kyy), Kyy.stride(0), jitter, n, _ptr(Rc), None, e, _ptr(f.A), f.ld,
                                          _ptr(f.winv), _ptr(work), _ptr(terms))
            _native.check(st, "gpn_lml_refine_dense")
            f.refined = True
        return terms[2:3].clone()

    @staticmethod
    def backward(ctx, grad_out):
        from . import _backward
        f = ctx.factor
        n, dy = f.n, f.e
        U = _backward._upper_inverse(f)
        Kinv = _backward._kinv_lower(f, U)[:n, :n]
        a_t = gemm_nt(f.A[n:], U, dy, n, round_up(n, 16), tri=TRI_B_UPPER)          # a^T = alpha^T U^T
        ap = torch.zeros(round_up(n, 16), round_up(dy, 16), dtype=torch.float64, device=f.device)
        ap[:n, :dy] = a_t.t()
        G = gemm_nt(ap, ap, n, n, round_up(dy, 16), alpha=0.5)                      # 1/2 a a^T
        G -= 0.5 * dy * (torch.tril(Kinv) + torch.tril(Kinv, -1).t())
        go = grad_out.reshape(())
        return (go * G if ctx.needs_input_grad[0] else None,
                -go * a_t.t() if ctx.needs_input_grad[1] else None,
                (go * G.diagonal().sum()).reshape(1) if ctx.needs_input_grad[2] else None)


# ----------------------------------------------------------------------------
# leave-one-out cross-validation (GPR(objective="loo")): csrc/loo.hip
# ----------------------------------------------------------------------------
def _rhs_rows(t, n):
    """a [dy, n] tensor as row-major right-hand sides: (tensor, leading dimension) -- a copy unless the rows are contiguous (a
    single row's stride says nothing)"""
    t = t.detach()
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < n):
        t = t.clone(memory_format=torch.contiguous_format)
    return t, max(t.stride(0), n)


def loo_terms(Kinv, at, n, dy, qt=None, want_q=True, want_var=True, want_rootd=True, want_value=True):
    """gpn_loo_terms: from the diagonal of Kinv (row-major) and at = a^T [dy, n] -> (qt [dy, n] = (y_i - mu_i)^T, var [n] = 1 / p_i,
    rootd [n] = sqrt(d_i), value 0-dim = L_LOO); an output that is not wanted is None.  qt given: a row-major buffer q^T is
    written into (a right-hand-side buffer for solve_right_lt).  No host synchronisation."""
    _req(Kinv, at, qt)
    dev = Kinv.device
    lib = _native.lib()
    at, ldat = _rhs_rows(at, n)

    def new(want, *shape):
        return torch.empty(shape, dtype=torch.float64, device=dev) if want else None

    if qt is None:
        qt = new(want_q, dy, n)
    work = new(True, max(1, int(lib.gpn_loo_terms_work_bytes(n)) // 8))
    var, rootd, value = new(want_var, n), new(want_rootd, n), new(want_value)
    st = lib.gpn_loo_terms(_stream(dev), n, dy, _ptr(Kinv), Kinv.stride(0), _ptr(at), ldat, _ptr(work), work.numel() * 8,
                           _ptr(qt), 0 if qt is None else max(qt.stride(0), n), _ptr(var), _ptr(rootd), _ptr(value))
    _native.check(st, "gpn_loo_terms")
    return qt, var, rootd, value


def loo_scale(Kinv, rootd, n, S):
    """gpn_loo_scale: S[:n, :n] = P diag(rootd), both triangles, from the lower triangle of Kinv; S: a ZEROED row-major buffer whose
    padding stays zero."""
    _req(Kinv, rootd, S)
    st = _native.lib().gpn_loo_scale(_stream(Kinv.device), n, _ptr(Kinv), Kinv.stride(0), _ptr(_c(rootd)), _ptr(S), S.stride(0))
    _native.check(st, "gpn_loo_scale")
    return S


def loo_grad(kind, X, variance, length_scales, Q, at, wt):
    """gpn_loo_grad: [2 + nls] = sum_ij G_ij dK_ij/d(variance, length_scales) (CONSTRAINED values) and tr G, with
    G = -Q + 1/2 (a w^T + w a^T); Q (row-major, lower triangle read), at = a^T and wt = w^T [dy, n]."""
    Xc, var, ls, args = _kargs(X, variance, length_scales)
    _req(Q, at, wt)
    dy, n = at.shape[0], Xc.shape[0]
    (at, ldat), (wt, ldwt) = _rhs_rows(at, n), _rhs_rows(wt, n)
    lib = _native.lib()
    nls = ls.numel()
    work = torch.empty(max(1, int(lib.gpn_loo_grad_work_bytes(Xc.shape[0], nls)) // 8), dtype=torch.float64, device=Xc.device)
    out = torch.empty(2 + nls, dtype=torch.float64, device=Xc.device)
    st = lib.gpn_loo_grad(_stream(Xc.device), KINDS[kind], *args, _ptr(Q), Q.stride(0), _ptr(at), ldat, _ptr(wt), ldwt, dy,
                          _ptr(work), work.numel() * 8, _ptr(out))
    _native.check(st, "gpn_loo_grad")
    return out


class LooState:
    """what the closed form reads off ONE factorisation f of Kyy with (L^-1 r)^T in its extra rows: Kinv (lower triangle of
    P = Kyy^-1 = U U^T), at = a^T = (P r)^T, qt = (y_i - mu_i)^T, var = 1 / p_i, rootd = sqrt(d_i), value = L_LOO and, with
    want_w, wt = w^T = (P q)^T -- q^T L^-T by the factor's right-solve, then one skinny contraction with U, the pair that gives
    a^T; computed here, while U is alive.  The tensors are this object's own: nothing refers to the factor buffer afterwards."""

    def __init__(self, f, want_w=True):
        from . import _backward
        n, dy = f.n, f.e
        self.n, self.dy, self.rows, self.ld = n, dy, f.rows, f.ld
        U = _backward._upper_inverse(f)
        self.Kinv = _backward._kinv_lower(f, U)
        kpad = round_up(n, 16)
        self.at = gemm_nt(f.A[n:], U, dy, n, kpad, tri=TRI_B_UPPER)                  # a^T = alpha^T U^T
        Bt = padded_like_factor(f, dy) if want_w else None
        qt, self.var, self.rootd, self.value = loo_terms(self.Kinv, self.at, n, dy, qt=Bt)
        self.wt = None
        if want_w:
            f.solve_right_lt(Bt, dy)                                                 # q^T L^-T = q^T U
            self.wt = gemm_nt(Bt, U, dy, n, kpad, tri=TRI_B_UPPER)                   # w^T = (q^T U) U^T
            qt = None                                                                # (overwritten by the solve)
        self.qt = qt

    def scaled_square(self):
        """S = P diag(sqrt d), both triangles, in a zeroed buffer with the factor's geometry"""
        return loo_scale(self.Kinv, self.rootd, self.n, zeros(self.rows, self.ld, self.Kinv.device))


class GPRLooLik(torch.autograd.Function):
    """The leave-one-out log predictive density L_LOO = sum_i log p(y_i | y_-i, X, theta) of the exact GP (Rasmussen & Williams
    5.4.2) as one autograd node with GPRLogLik's inputs; output shape (1,).
    Forward: the factorisation of GPRLogLik (kernel_factor: the same jitter ladder, the model's reusable factor buffer), U = L^-T,
    P = U U^T, a^T, the per-point terms (gpn_loo_terms) and w = P q.  The node keeps P, a^T, w^T and sqrt(d) PRIVATELY: its
    backward never reads the shared factor buffer, so a later forward into that buffer cannot invalidate it.
    Backward: S = P diag(sqrt d) (gpn_loo_scale), Q = S S^T (one lower contraction), the sweep gpn_loo_grad.
    Memory: four N x N buffers at the peak of either pass (forward: factor, U, the inversion's workspace, P; backward: factor, P, S, Q)."""

    @staticmethod
    def forward(ctx, X, R, variance, length_scales, noise, kind, holder):
        n = R.shape[0]
        if X.shape[0] != n:
            raise ValueError("X and Y must have same # data.")
        f = kernel_factor(kind, X, variance, length_scales, noise, R=R, factor=holder.get("factor"))
        holder["factor"] = f
        ctx.kind = kind
        ctx.state = LooState(f)
        ctx.save_for_backward(X, variance, length_scales)
        return ctx.state.value.reshape(1)

    @staticmethod
    def backward(ctx, grad_out):
        X, variance, length_scales = ctx.saved_tensors
        s = ctx.state
        n = s.n
        S = s.scaled_square()
        Q = torch.empty(round_up(max(n, 1), 64), s.ld, dtype=torch.float64, device=S.device)
        gemm_nt(S, S, n, n, round_up(n, 16), C=Q, lower=True)                       # Q = P diag(d) P, lower triangle
        out = loo_grad(ctx.kind, X, variance, length_scales, Q, s.at, s.wt)
        nls = length_scales.numel()
        go = grad_out.reshape(())
        return (None, -go * s.wt.t() if ctx.needs_input_grad[1] else None, go * out[0:1], go * out[1:1 + nls].reshape(length_scales.shape),
                go * out[1 + nls:2 + nls], None, None)


# ---- the same in lock step: `batch` equal-shape models per launch (gpn_loo_*_batched: the single kernels with the model on the grid's
# y dimension).  Operands are device ADDRESSES (or tensors) with a leading dimension and a model stride in doubles, because they live
# inside gpn_lml_kinv_batched's workspace; every row of every result is bit-identical to the single wrapper called on that model.
def loo_terms_batched(batch, n, dy, Kinv, ldk, sK, at, ldat, sAt, device, qt=None, ldqt=0, sQt=0, want_var=True, want_rootd=True,
                      want_value=True):
    """gpn_loo_terms_batched -> (var [batch, n], rootd [batch, n], value [batch]); qt (address / tensor, ldqt, sQt): q^T of model b is
    written at qt + b sQt, None: not wanted."""
    lib = _native.lib()

    def new(want, *shape):
        return torch.empty(shape, dtype=torch.float64, device=device) if want else None

    work = new(True, max(1, int(lib.gpn_loo_terms_batched_work_bytes(n, batch)) // 8))
    var, rootd, value = new(want_var, batch, n), new(want_rootd, batch, n), new(want_value, batch)
    st = lib.gpn_loo_terms_batched(_stream(device), batch, n, dy, _addr(Kinv), ldk, sK, _addr(at), ldat, sAt, _ptr(work), work.numel() * 8,
                                   None if qt is None else _addr(qt), ldqt, sQt, _ptr(var), _ptr(rootd), _ptr(value))
    _native.check(st, "gpn_loo_terms_batched")
    return var, rootd, value


def loo_scale_batched(batch, n, Kinv, ldk, sK, rootd, S, lds, sS):
    """gpn_loo_scale_batched: S_b[:n, :n] = P_b diag(rootd[b]), both triangles; rootd [batch, n]; Kinv, S: addresses / tensors."""
    _req(rootd)
    st = _native.lib().gpn_loo_scale_batched(_stream(rootd.device), batch, n, _addr(Kinv), ldk, sK, _ptr(_c(rootd)), _addr(S), lds, sS)
    _native.check(st, "gpn_loo_scale_batched")


def loo_grad_batched(kind, X, variance, length_scales, Q, ldq, sQ, at, ldat, sAt, wt, ldwt, sWt, dy, work=None):
    """gpn_loo_grad_batched: [batch, 2 + nls], row b = loo_grad of model b (Q, at, wt: addresses / tensors with their leading dimension
    and model stride)."""
    Xc, var, ls, batch, n, args = _kargs_batched(X, variance, length_scales)
    lib = _native.lib()
    nls = ls.shape[1]
    need = max(1, int(lib.gpn_loo_grad_batched_work_bytes(n, nls, batch)) // 8)
    if work is None or work.numel() < need:
        work = torch.empty(need, dtype=torch.float64, device=Xc.device)
    out = torch.empty(batch, 2 + nls, dtype=torch.float64, device=Xc.device)
    st = lib.gpn_loo_grad_batched(_stream(Xc.device), KINDS[kind], *args, _addr(Q), ldq, sQ, _addr(at), ldat, sAt, _addr(wt), ldwt, sWt, dy,
                                  _ptr(work), work.numel() * 8, _ptr(out))
    _native.check(st, "gpn_loo_grad_batched")
    return out


class LooGroupState:
    """LooState for the `batch` models of one lock-step group, every launch once over all of them: the factors of
    lml_forward_batched (holder["fb"]), gpn_lml_kinv_batched's workspace `wk` (per model: U at offset 0 -- later S --, P, a^T), q^T
    into right-hand-side buffers padded like the factor, the right-solve and the skinny contraction with U for w^T.  rootd, wt and
    value are this object's own tensors; P and a^T stay in the holder's workspace, valid while holder["loo_generation"] == generation.
    No host synchronisation (the caller reads fb.info)."""

    def __init__(self, kind, X, R, variance, length_scales, noise, holder):
        lib = _native.lib()
        batch, n, dy = int(variance.numel()), R.shape[-2], R.shape[-1]
        dev = X.device
        fb, _terms = lml_forward_batched(kind, X, R, variance, length_scales, noise, fb=holder.get("fb"), refine=False)
        holder["fb"] = fb
        holder["loo_generation"] = self.generation = holder.get("loo_generation", 0) + 1
        self.holder, self.fb, self.batch, self.n, self.dy = holder, fb, batch, n, dy
        lay = (ctypes.c_int64 * 4)()
        _native.check(lib.gpn_lml_kinv_layout(n, dy, lay), "gpn_lml_kinv_layout")
        self.ld, self.koff, self.aoff, self.stride = (int(v) for v in lay)
        need = max(1, int(lib.gpn_lml_kinv_batched_work_bytes(n, dy, batch)) // 8)
        if fb._backward_work is None or fb._backward_work.numel() < need:
            fb._backward_work = torch.empty(need, dtype=torch.float64, device=dev)
            holder["loo_dirty"] = False
        self.wk = wk = fb._backward_work
        s = _stream(dev)
        if holder.get("loo_dirty") and n > 256 and n % LEAF == 0:
            # an earlier backward left S where U goes: the inversion gets the zeroed slot it is documented to start from (at the other
            # sizes gpn_lml_kinv_batched clears the slot itself)
            urows = int(lib.gpn_factor_rows(n, 0))
            for b in range(batch):
                _native.check(lib.gpn_fill_zero(s, wk.data_ptr() + 8 * b * self.stride, 8 * urows * self.ld), "gpn_fill_zero")
            holder["loo_dirty"] = False
        _native.check(lib.gpn_lml_kinv_batched(s, batch, n, _ptr(fb.A), fb.ld, fb.sA, _ptr(fb.winv), fb.sW, dy, _ptr(wk)), "gpn_lml_kinv_batched")
        base = wk.data_ptr()
        self.kinv_addr, self.at_addr = base + 8 * self.koff, base + 8 * self.aoff
        brows = round_up(max(dy, 1), LEAF)
        Bt = holder.get("loo_rhs")
        if Bt is None or tuple(Bt.shape) != (batch * brows, fb.ld) or Bt.device != dev:
            Bt = holder["loo_rhs"] = torch.empty(batch * brows, fb.ld, dtype=torch.float64, device=dev)
        _native.check(lib.gpn_fill_zero(s, _ptr(Bt), Bt.numel() * 8), "gpn_fill_zero")
        self.var, self.rootd, self.value = loo_terms_batched(batch, n, dy, self.kinv_addr, self.ld, self.stride, self.at_addr, self.ld,
                                                             self.stride, dev, qt=Bt, ldqt=fb.ld, sQt=brows * fb.ld)
        self.wt = torch.empty(batch, dy, n, dtype=torch.float64, device=dev)
        if n:
            st = lib.gpn_trsm_right_lt_batched(s, _ptr(fb.A), n, fb.ld, fb.sA, _ptr(fb.winv), fb.sW, _ptr(Bt), dy, fb.ld, brows * fb.ld, batch)
            _native.check(st, "gpn_trsm_right_lt_batched")                            # q^T L^-T = q^T U
            st = lib.gpn_gemm_nt_batched(s, dy, n, round_up(n, 16), 1.0, _ptr(Bt), fb.ld, brows * fb.ld, _addr(base), self.ld, self.stride,
                                         0.0, _ptr(self.wt), n, dy * n, 0, TRI_B_UPPER, batch)
            _native.check(st, "gpn_gemm_nt_batched")                                  # w^T = (q^T U) U^T

    def valid(self):
        return self.holder.get("loo_generation") == self.generation and self.holder.get("fb") is self.fb and self.fb._backward_work is self.wk

    def grads(self, kind, X, variance, length_scales):
        """[batch, 2 + nls]: gpn_loo_scale_batched (S into U's slot: U is not read again), ONE lower contraction Q = S S^T over the
        group, gpn_loo_grad_batched"""
        lib = _native.lib()
        batch, n, dy, holder = self.batch, self.n, self.dy, self.holder
        dev = self.wk.device
        base = self.wk.data_ptr()
        qrows = round_up(max(n, 1), 64)
        Q = holder.get("loo_q")
        if Q is None or tuple(Q.shape) != (batch, qrows, self.ld) or Q.device != dev:
            Q = holder["loo_q"] = torch.empty(batch, qrows, self.ld, dtype=torch.float64, device=dev)
        holder["loo_dirty"] = True
        loo_scale_batched(batch, n, self.kinv_addr, self.ld, self.stride, self.rootd, base, self.ld, self.stride)
        if n:
            st = lib.gpn_gemm_nt_batched(_stream(dev), n, n, round_up(n, 16), 1.0, _addr(base), self.ld, self.stride, _addr(base), self.ld, self.stride,
                                         0.0, _ptr(Q), self.ld, qrows * self.ld, 1, 0, batch)
            _native.check(st, "gpn_gemm_nt_batched")
        nls = length_scales.reshape(batch, -1).shape[1]
        need = max(1, int(lib.gpn_loo_grad_batched_work_bytes(n, nls, batch)) // 8)
        work = holder.get("loo_sweep")
        if work is None or work.numel() < need or work.device != dev:
            work = holder["loo_sweep"] = torch.empty(need, dtype=torch.float64, device=dev)
        return loo_grad_batched(kind, X, variance, length_scales, Q, self.ld, qrows * self.ld, self.at_addr, self.ld, self.stride,
                                self.wt, n, dy * n, dy, work=work)


class BatchedGPRLooLik(torch.autograd.Function):
    """GPRLooLik for `batch` independent models of one shape in LOCK STEP (restarts and kernel choices of a leave-one-out fit): the
    inputs of BatchedGPRLogLik without n_of -> L_LOO [batch].  Forward: LooGroupState (gpn_lml_forward_batched, gpn_lml_kinv_batched,
    gpn_loo_terms_batched, gpn_trsm_right_lt_batched + gpn_gemm_nt_batched); ONE read of `info` for the group; a model whose
    factorisation reports info != 0 is replayed ALONE through kernel_factor's jitter ladder + LooState, and its backward runs on that
    private state.  Backward: gpn_loo_scale_batched, one gpn_gemm_nt_batched (lower), gpn_loo_grad_batched, dL/dR = -w.  The state
    lives in the group's cached buffers under a generation stamp: a backward that finds it moved (a later forward reused the buffers)
    rebuilds its state privately.  Values and gradients are bit-identical, model by model, to GPRLooLik.
    Memory per model: the factor, U (later S), P and Q -- four padded N x N matrices (models/_loo_lockstep.per_model_bytes)."""

    @staticmethod
    def forward(ctx, X, R, variance, length_scales, noise, kind, holder):
        batch = int(variance.numel())
        if X.shape[-2] != R.shape[-2]:
            raise ValueError("X and Y must have same # data.")
        state = LooGroupState(kind, X, R, variance, length_scales, noise, holder)
        out = state.value.clone()
        info = state.fb.info.cpu()                   # ONE read-back for the group
        replayed = {}
        for b in (torch.nonzero(info).reshape(-1).tolist() if bool(info.any()) else ()):
            f = kernel_factor(kind, X if X.dim() == 2 else X[b], variance.reshape(batch)[b:b + 1], length_scales.reshape(batch, -1)[b],
                              noise.reshape(batch)[b:b + 1], R=R if R.dim() == 2 else R[b])
            replayed[b] = (LooState(f), f.jitter_rung)
            out[b] = replayed[b][0].value
        holder["loo_replayed"] = {b: rung for b, (_s, rung) in replayed.items()}
        ctx.kind, ctx.state, ctx.replayed = kind, state, replayed
        ctx.save_for_backward(X, R, variance, length_scales, noise)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        X, R, variance, length_scales, noise = ctx.saved_tensors
        batch = int(variance.numel())
        state = ctx.state
        if not state.valid():
            # the group's buffers were reused by a later forward: this node's P and a^T are gone, rebuild them in buffers of its own
            state = LooGroupState(ctx.kind, X, R, variance, length_scales, noise, {})
        n, dy = state.n, state.dy
        grads = state.grads(ctx.kind, X, variance, length_scales)
        nls = grads.shape[1] - 2
        need_r = ctx.needs_input_grad[1]
        g_R = (-state.wt).transpose(1, 2) if need_r else None                        # dL/dR = -w, [batch, n, dy] (a tensor of its own)
        for b, (s, _rung) in ctx.replayed.items():
            S = s.scaled_square()
            Q = torch.empty(round_up(max(n, 1), 64), s.ld, dtype=torch.float64, device=S.device)
            gemm_nt(S, S, n, n, round_up(n, 16), C=Q, lower=True)
            grads[b] = loo_grad(ctx.kind, X if X.dim() == 2 else X[b], variance.reshape(batch)[b:b + 1], length_scales.reshape(batch, -1)[b],
                                Q, s.at, s.wt)
            if need_r:
                g_R[b] = -s.wt.t()
        go = grad_out.reshape(batch)
        g_resid = None
        if need_r:
            g_resid = go[:, None, None] * g_R
            if R.dim() == 2:
                g_resid = g_resid.sum(0)
        return (None, g_resid, (go * grads[:, 0]).reshape(variance.shape), (go[:, None] * grads[:, 1:1 + nls]).reshape(length_scales.shape),
                (go * grads[:, 1 + nls]).reshape(noise.shape), None, None)


class DenseLooLik(torch.autograd.Function):
    """GPRLooLik for a kernel matrix that arrives as a dense tensor (Sum / Product / Linear / White ... kernels), the way DenseLogLik
    serves the LML: Kyy = K + noise I is factorised natively, P, the terms and S are GPRLooLik's, Q = S S^T is a full contraction,
    the rank terms 1/2 (a w^T + w a^T) = 1/2 [a w] [w a]^T one skinny one, and dL_LOO/dK = G = -Q + 1/2 (a w^T + w a^T) goes back
    to autograd as a dense [n, n] gradient for the kernels' own backward sweeps (-w for R, tr G for the noise)."""

    @staticmethod
    def forward(ctx, K, R, noise):
        Kyy = K.detach().clone()
        Kyy.diagonal().add_(noise.detach()[0])
        ctx.state = LooState(cholesky_factor(Kyy, rhs=R))
        return ctx.state.value.reshape(1)

    @staticmethod
    def backward(ctx, grad_out):
        s = ctx.state
        n, dy = s.n, s.dy
        S = s.scaled_square()
        G = gemm_nt(S, S, n, n, round_up(n, 16))                                    # Q, both triangles
        left = torch.zeros(round_up(n, 16), round_up(2 * dy, 16), dtype=torch.float64, device=S.device)
        right = torch.zeros_like(left)
        left[:n, :dy], left[:n, dy:2 * dy] = s.at.t(), s.wt.t()
        right[:n, :dy], right[:n, dy:2 * dy] = s.wt.t(), s.at.t()
        gemm_nt(left, right, n, n, round_up(2 * dy, 16), alpha=0.5, beta=-1.0, C=G)  # G = 1/2 (a w^T + w a^T) - Q
        go = grad_out.reshape(())
        return (go * G if ctx.needs_input_grad[0] else None,
                -go * s.wt.t() if ctx.needs_input_grad[1] else None,
                (go * G.diagonal().sum()).reshape(1) if ctx.needs_input_grad[2] else None)


# ----------------------------------------------------------------------------
# k-fold cross-validation in closed form (GPR(objective="kfold")): csrc/kfold.hip
# ----------------------------------------------------------------------------
KFOLD_PAD_FACTOR = 4     # a partition is refused when k * round_up(m_max, 16) > KFOLD_PAD_FACTOR * round_up(n, 16) (FoldTable)


class FoldTable:
    """A partition of range(n) into k >= 2 folds as the kernels read it: off [k + 1] and idx [n], int32 on `device` (fold f =
    idx[off[f] : off[f + 1]], in the order given), m_max the largest fold.  folds: an int k (np.array_split(np.arange(n), k):
    contiguous blocks in data order, no shuffling) or a sequence of integer index arrays; anything that is not a partition with
    at least two non-empty folds raises ValueError.  Every fold is padded to m_max: a partition with k * round_up(m_max, 16) >
    4 round_up(n, 16) (all-singleton folds among them) would more than quadruple an N x N buffer -- [round_up(n, 16), k *
    round_up(m_max, 16)] is the column buffer of the backward -- and raises NotImplementedError.  (Both sides count padded rows:
    against the bare n the 16-row granule alone would refuse every partition of fewer than 8 points.)"""

    def __init__(self, folds, n, device=None):
        import numpy as np
        n = int(n)
        if folds is None:
            raise ValueError("objective='kfold' needs folds: an int k >= 2 or a sequence of index arrays that partition range(n)")
        if isinstance(folds, (int, np.integer)) and not isinstance(folds, bool):
            k = int(folds)
            if k < 2 or k > n:
                raise ValueError("folds: an int k must satisfy 2 <= k <= n = %d; got %d" % (n, k))
            parts = np.array_split(np.arange(n), k)
        else:
            try:
                parts = [np.asarray(p.detach().cpu() if torch.is_tensor(p) else p) for p in folds]
            except TypeError:
                raise ValueError("folds must be an int or a sequence of integer index arrays; got %r" % (folds,))
            if len(parts) < 2:
                raise ValueError("folds: at least two folds are needed; got %d" % len(parts))
            for p in parts:
                if p.ndim != 1 or p.size == 0:
                    raise ValueError("folds: every fold is a non-empty 1-D index array")
                if p.dtype.kind not in "iu":
                    raise ValueError("folds: index arrays must hold integers; got dtype %s" % p.dtype)
            flat = np.concatenate(parts).astype(np.int64)
            if flat.size != n or flat.min() < 0 or flat.max() >= n or np.unique(flat).size != n:
                raise ValueError("folds must partition range(%d): every index exactly once" % n)
        sizes = [int(p.size) for p in parts]
        self.n, self.k, self.sizes, self.m_max = n, len(parts), tuple(sizes), max(sizes)
        if self.k * round_up(self.m_max, 16) > KFOLD_PAD_FACTOR * round_up(n, 16):
            raise NotImplementedError(
                "folds: padding %d folds to the largest (%d points) would more than quadruple an N x N buffer at n = %d; "
                "for (nearly) singleton folds use objective=\"loo\"" % (self.k, self.m_max, n))
        self.parts = [p.astype(np.int64) for p in parts]
        self._off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32)
        self._idx = torch.tensor(np.concatenate(self.parts), dtype=torch.int32)
        self._on = {}
        if device is not None:
            self.on(device)

    def on(self, device):
        """(off, idx) on `device` (copied once per device)"""
        device = torch.device(device)
        if device not in self._on:
            self._on[device] = (self._off.to(device), self._idx.to(device))
        return self._on[device]


def kfold_gather(Kinv, at, n, dy, table, fb):
    """gpn_kfold_gather: P[I_f, I_f], the identity padding and a_I^T into the k ZEROED factor buffers of the FactorBatch fb"""
    _req(Kinv, at)
    at, ldat = _rhs_rows(at, n)
    off, idx = table.on(Kinv.device)
    st = _native.lib().gpn_kfold_gather(_stream(Kinv.device), n, dy, _ptr(Kinv), Kinv.stride(0), _ptr(at), ldat, table.k, _ptr(off), _ptr(idx),
                                        table.m_max, _ptr(fb.A), fb.ld, fb.sA)
    _native.check(st, "gpn_kfold_gather")
    return fb


def kfold_columns(Kinv, n, table):
    """gpn_kfold_columns: P[:, I_f] as full columns -> [k, round_up(n, 16), round_up(m_max, 16)], zero padded"""
    _req(Kinv)
    off, idx = table.on(Kinv.device)
    C = torch.empty(table.k, round_up(n, 16), round_up(table.m_max, 16), dtype=torch.float64, device=Kinv.device)
    st = _native.lib().gpn_kfold_columns(_stream(Kinv.device), n, _ptr(Kinv), Kinv.stride(0), table.k, _ptr(off), _ptr(idx), table.m_max,
                                         _ptr(C), C.stride(1), C.stride(0))
    _native.check(st, "gpn_kfold_columns")
    return C


def kfold_factorise(fb):
    """the k gathered fold blocks factorised in lock step (gpn_potrf_lower_batched: beta_f^T = a_I^T L_f^-T in the extra rows) ->
    (out3 [k, 3] of gpn_lml_reduce_batched, U [k, rows, ld] = L_f^-T of gpn_trtri_upper_batched).  fb.info is left on the device."""
    lib = _native.lib()
    dev = fb.A.device
    fb.info.zero_()
    st = lib.gpn_potrf_lower_batched(_stream(dev), _ptr(fb.A), fb.n, fb.e, fb.ld, fb.sA, _ptr(fb.winv), fb.sW, _ptr(fb.info), fb.batch)
    _native.check(st, "gpn_potrf_lower_batched")
    st = lib.gpn_lml_reduce_batched(_stream(dev), _ptr(fb.A), fb.n, fb.e, fb.ld, fb.sA, _ptr(fb.out), fb.batch)
    _native.check(st, "gpn_lml_reduce_batched")
    U = zeros(fb.batch * fb.rows, fb.ld, dev)
    S = zeros(fb.batch * fb.rows, fb.ld, dev) if fb.n > 2 * LEAF else None
    st = lib.gpn_trtri_upper_batched(_stream(dev), _ptr(fb.A), fb.n, fb.ld, fb.sA, _ptr(fb.winv), fb.sW, _ptr(U), fb.ld, fb.sA,
                                     _ptr(S), fb.ld, fb.sA, fb.batch)
    _native.check(st, "gpn_trtri_upper_batched")
    if S is not None:
        S.record_stream(torch.cuda.current_stream(dev))
    return fb.out, U


def kfold_terms(table, n, dy, fb, U, out3=None, info=None, qt=None, want_q=True, want_var=True, want_w=True, want_value=True):
    """gpn_kfold_terms -> (qt [dy, n] = (y - mu)^T and var [n] in DATA order, Wt [k, round_up(m_max + dy, 16), round_up(m_max, 16)]
    = W_f^T, value 0-dim = L_kfold); an output that is not wanted is None.  qt given: a row-major buffer q^T is written into."""
    lib = _native.lib()
    dev = fb.A.device
    off, idx = table.on(dev)
    k, m = table.k, table.m_max

    def new(want, *shape):
        return torch.empty(shape, dtype=torch.float64, device=dev) if want else None

    if qt is None:
        qt = new(want_q, dy, n)
    var, value = new(want_var, n), new(want_value)
    Wt = zeros(k * round_up(m + dy, 16), round_up(m, 16), dev) if want_w else None
    st = lib.gpn_kfold_terms(_stream(dev), n, dy, k, _ptr(off), _ptr(idx), m, _ptr(U), fb.ld, fb.sA, _ptr(fb.A), fb.ld, fb.sA,
                             _ptr(out3), _ptr(info), _ptr(qt), 0 if qt is None else max(qt.stride(0), n), _ptr(var),
                             _ptr(Wt), 0 if Wt is None else Wt.stride(0), round_up(m + dy, 16) * round_up(m, 16), _ptr(value))
    _native.check(st, "gpn_kfold_terms")
    return qt, var, Wt, value


class KFoldState:
    """what the k-fold closed form reads off ONE factorisation f of Kyy with (L^-1 r)^T in its extra rows and a FoldTable: Kinv
    (lower triangle of P = Kyy^-1 = U U^T, formed exactly as LooState forms it), at = a^T, the k fold blocks P[I_f, I_f] gathered
    into equal-shape factor buffers and factorised in lock step WITHOUT jitter, qt = (y - mu)^T and var = diag Sigma_f in data
    order, value = L_kfold and, with want_w, Wt = W_f^T and wt = w^T = (P q)^T (the factor's right-solve plus a skinny contraction
    with U, LooState's route).  bad: some fold's factorisation reported info != 0 (ONE host read for the group of folds): value is
    NaN and so is every gradient; nothing is clamped.  The tensors are this object's own: nothing refers to the factor buffer
    afterwards.  The number of launches depends on neither k nor n."""

    def __init__(self, f, table, want_w=True):
        from . import _backward
        n, dy = f.n, f.e
        if table.n != n:
            raise ValueError("folds partition range(%d) but the data have %d rows" % (table.n, n))
        self.n, self.dy, self.rows, self.ld, self.table = n, dy, f.rows, f.ld, table
        U = _backward._upper_inverse(f)
        self.Kinv = _backward._kinv_lower(f, U)
        kpad = round_up(n, 16)
        self.at = gemm_nt(f.A[n:], U, dy, n, kpad, tri=TRI_B_UPPER)                  # a^T = alpha^T U^T
        fb = FactorBatch(table.k, table.m_max, dy, f.device)
        kfold_gather(self.Kinv, self.at, n, dy, table, fb)
        out3, Uf = kfold_factorise(fb)
        Bt = padded_like_factor(f, dy) if want_w else None
        qt, self.var, self.Wt, self.value = kfold_terms(table, n, dy, fb, Uf, out3=out3, info=fb.info, qt=Bt, want_w=want_w)
        self.fold_terms = out3                                                       # [k, 3]: sum log L_f,ii, ||beta_f||^2, (unused)
        self.wt = None
        if want_w:
            f.solve_right_lt(Bt, dy)                                                 # q^T L^-T = q^T U
            self.wt = gemm_nt(Bt, U, dy, n, kpad, tri=TRI_B_UPPER)                   # w^T = (q^T U) U^T
            qt = None                                                                # (overwritten by the solve)
        self.qt = qt
        self.bad = bool((fb.info != 0).any().item())                                 # the one host read of the folds' info

    def scaled_columns(self):
        """S = [P[:, I_f] W_f]_f, [round_up(n, 16), k * round_up(m_max + dy, 16)]: gpn_kfold_columns and ONE strided-batch
        contraction; Q = P D P = S S^T"""
        t, n = self.table, self.n
        wp, mp = round_up(t.m_max + self.dy, 16), round_up(t.m_max, 16)
        C = kfold_columns(self.Kinv, n, t)
        S = torch.empty(round_up(n, 16), t.k * wp, dtype=torch.float64, device=C.device)
        st = _native.lib().gpn_gemm_nt_batched(_stream(C.device), n, wp, mp, 1.0, _ptr(C), mp, C.stride(0), _ptr(self.Wt), mp, wp * mp,
                                               0.0, _ptr(S), S.stride(0), wp, 0, 0, t.k)
        _native.check(st, "gpn_gemm_nt_batched")
        return S


def _nan_like(t):
    return torch.full_like(t, float("nan"))


class GPRKFoldLik(torch.autograd.Function):
    """The k-fold log predictive density L_kfold = sum_f log p(y_I | y_-I, X, theta) of the exact GP in closed form from the diagonal
    blocks of P = Kyy^-1, as one autograd node with GPRLooLik's inputs plus the FoldTable; output shape (1,).
    Forward: the factorisation of GPRLogLik (kernel_factor: the same jitter ladder, the model's reusable factor buffer), then
    KFoldState.  The node keeps P, a^T, w^T, W^T PRIVATELY: its backward never reads the shared factor buffer.  P_f gets no jitter:
    a fold whose factorisation reports info != 0 makes the value and every gradient NaN.
    Backward: gpn_kfold_columns, S = [P[:, I_f] W_f] (one strided-batch contraction), Q = S S^T (one lower contraction), the sweep
    gpn_loo_grad; dL/dR = -w.
    Memory, in N x N: forward peak 4 (factor, U, the inversion's workspace, P; the folds' buffers add about 3 / k); backward:
    factor, P, the column buffer (k round_up(m_max, 16) / n: about 1 for near-equal folds, at most 4 by FoldTable's rule) and S
    (about 1) during the block product, then -- the column buffer released -- factor, P, S, Q: a peak of about 4 for near-equal
    folds, plus W^T (1 / k)."""

    @staticmethod
    def forward(ctx, X, R, variance, length_scales, noise, kind, holder, table):
        n = R.shape[0]
        if X.shape[0] != n:
            raise ValueError("X and Y must have same # data.")
        f = kernel_factor(kind, X, variance, length_scales, noise, R=R, factor=holder.get("factor"))
        holder["factor"] = f
        ctx.kind = kind
        ctx.state = KFoldState(f, table)
        ctx.save_for_backward(X, R, variance, length_scales, noise)
        return ctx.state.value.reshape(1)

    @staticmethod
    def backward(ctx, grad_out):
        X, R, variance, length_scales, noise = ctx.saved_tensors
        s = ctx.state
        if s.bad:
            # a fold block was not positive definite: the value is NaN and so is every gradient
            return (None, _nan_like(R) if ctx.needs_input_grad[1] else None, _nan_like(variance), _nan_like(length_scales), _nan_like(noise),
                    None, None, None)
        n = s.n
        S = s.scaled_columns()
        Q = torch.empty(round_up(max(n, 1), 64), s.ld, dtype=torch.float64, device=S.device)
        gemm_nt(S, S, n, n, S.shape[1], C=Q, lower=True)                             # Q = P D P, lower triangle
        del S
        out = loo_grad(ctx.kind, X, variance, length_scales, Q, s.at, s.wt)
        nls = length_scales.numel()
        go = grad_out.reshape(())
        return (None, -go * s.wt.t() if ctx.needs_input_grad[1] else None, go * out[0:1], go * out[1:1 + nls].reshape(length_scales.shape),
                go * out[1 + nls:2 + nls], None, None, None)


class DenseKFoldLik(torch.autograd.Function):
    """GPRKFoldLik for a kernel matrix that arrives as a dense tensor (Sum / Product / Linear / White ... kernels), as DenseLooLik
    serves the leave-one-out objective: the same native steps, Q = S S^T as a full contraction, and dL_kfold/dK = G goes back to
    autograd as a dense [n, n] gradient (-w for R, tr G for the noise).  Memory: GPRKFoldLik's plus the dense K and G."""

    @staticmethod
    def forward(ctx, K, R, noise, table):
        Kyy = K.detach().clone()
        Kyy.diagonal().add_(noise.detach()[0])
        ctx.state = KFoldState(cholesky_factor(Kyy, rhs=R), table)
        ctx.save_for_backward(K, R, noise)
        return ctx.state.value.reshape(1)

    @staticmethod
    def backward(ctx, grad_out):
        K, R, noise = ctx.saved_tensors
        s = ctx.state
        if s.bad:
            return (_nan_like(K) if ctx.needs_input_grad[0] else None, _nan_like(R) if ctx.needs_input_grad[1] else None,
                    _nan_like(noise) if ctx.needs_input_grad[2] else None, None)
        n, dy = s.n, s.dy
        S = s.scaled_columns()
        G = gemm_nt(S, S, n, n, S.shape[1])                                          # Q, both triangles
        del S
        left = torch.zeros(round_up(n, 16), round_up(2 * dy, 16), dtype=torch.float64, device=G.device)
        right = torch.zeros_like(left)
        left[:n, :dy], left[:n, dy:2 * dy] = s.at.t(), s.wt.t()
        right[:n, :dy], right[:n, dy:2 * dy] = s.wt.t(), s.at.t()
        gemm_nt(left, right, n, n, round_up(2 * dy, 16), alpha=0.5, beta=-1.0, C=G)  # G = 1/2 (a w^T + w a^T) - Q
        go = grad_out.reshape(())
        return (go * G if ctx.needs_input_grad[0] else None,
                -go * s.wt.t() if ctx.needs_input_grad[1] else None,
                (go * G.diagonal().sum()).reshape(1) if ctx.needs_input_grad[2] else None, None)


LOG_2PI = math.log(2.0 * math.pi)
