"""
Sparse GP regression: VFE (Titsias' collapsed bound), gptorch/models/sparse_gpr.py:22-195,
BASELINE config 5 / SURVEY 8(f)-1 (N = 1e6 points, M = 4096 inducing points).

Forward.  Everything N-sized is STREAMED in row chunks of x (CHUNK_ROWS at a time), so the
M x N matrices Kuf / A of the reference are never held -- only two chunk-sized scratch
buffers and a handful of M x M matrices live in HBM -- and every contraction is the NT
fp64-MFMA form of the library:

    per chunk c:  A_c^T = K(x_c, Z) L^-T        [nc, M]  assembly + in-place right-solve
                  A_c   = (A_c^T)^T             [M, nc]  HBM-bound transpose
                  AAT  += A_c A_c^T / s2        [M, M]   SYRK (lower), beta = 1
                  Aerr += A_c err_c             [M, dy]
    then          B = AAT + I = LB LB^T, with (Aerr)^T carried as the factor's extra rows,
                  so c * s2 = LB^-1 Aerr falls out of the factorisation.

Backward (closed form, verified against autograd through the reference's op chain in
tests/golden/make_golden.py; the reference gets it from autograd through two Cholesky
backwards and two M x N triangular-solve backwards).  With p = dy, s = s2,
beta = B^-1 A err / s, gamma = L^-T beta:

    dF/dKuu = L^-T [ p/2 (2I - B^-1 - B) - 1/2 beta beta^T ] L^-1                (M x M)
    dF/dKuf = 1/s ( P Kuf + gamma err^T ),  P = L^-T [ p (I - B^-1) - beta beta^T ] L^-1
    dF/ds   = p/(2s) (M - tr B^-1) - |c|^2/s + beta^T (B - I) beta/(2s) - p tr(AAT)/(2s)
              - p N/(2s) + (|err|^2 + p tr Kff)/(2 s^2),        dF/dvar += -p N/(2s)

so the N-sized part is ONE dense [nc, M] x [M, M] contraction per chunk (no solve), followed
by the HBM-bound sweeps that contract dF/dKuf with dK/dtheta (gpn_kernel_grad) and dK/dZ
(gpn_kernel_grad_x2).  Forward + backward cost 4 N M^2 flops instead of holding 2 x 33 GB.

Why the forward keeps the N-sized solve: A A^T = L^-1 (Kuf Kfu) L^-T would halve the forward
flops (no N x M TRSM), but only the Gram form A A^T of a COMPUTED A is positive semi-definite
by construction; the sandwich loses definiteness by ~eps |Kuf|^2 / lambda_min(Kuu), and at
config 5 (4096 inducing points, Kuu at the edge of the jitter ladder) chol(B) then fails on
every rung.  Measured, not assumed (round 1).

SVGP (sparse_gpr.py:198-381) follows VFE below: a minibatch bound over the same M-sized algebra with its own row kernels
(csrc/svgp.hip).  FITC (sparse_gpr.py:76-90, an empty class in the reference) lives in models/_fitc.py: the same streamed pipeline
(_stream_gram) with its own row kernels (csrc/fitc.hip) between the right-solve and the accumulation.
"""
import functools
import math

import numpy as np
import torch

from .. import _backward, _ops
from ..mean_functions import Zero
from ..param import Param
from ..util import as_tensor
from .base import GPModel

CHUNK_ROWS = 65536   # rows of x per streamed chunk (scratch: 2 x CHUNK_ROWS x ld(M) x 8 B)
# Measured alternative, OFF by default (round 3): from INVERSE_MIN_M inducing points on (and N >= 4 M) form W = L^-1 once per
# evaluation (M^3/3 flops) and compute every chunk's A_c = L^-1 Kuf_c as W Kuf_c -- already in the [M, rows] layout the A A^T
# accumulation reads, so the right-solve recursion AND the transpose go.  Same bound to 8e-12 relative at config 5, gradients
# equal to the solve path's wherever Kuu is not numerically singular (tests: test_vfe_inverse_path_vs_oracle) -- but not
# faster: as ONE K-clipped launch per chunk 0.610 s (uneven tiles, dealt round-robin over the XCDs), as block rows of
# INVERSE_BLOCK rows with plain launches 0.561-0.564 s, against 0.549-0.552 s for the right-solve (same box, interleaved;
# profiles/r3_vfe_inverse_ab.txt): with two chunk pipelines in flight the bound is throughput-bound at ~62 TFLOP/s and the
# inverse form carries 6 % more flops.
INVERSE_MIN_M = int(__import__('os').environ.get('GPN_VFE_INVERSE_MIN_M', 1 << 62))
INVERSE_BLOCK = int(__import__('os').environ.get('GPN_VFE_INVERSE_BLOCK', 512))
# N-sharding over the GPUs of a node: when set to a torch.distributed process group
# (or True for the default group) every rank holds a ROW SHARD of (x, y) and the same Z and
# hyper-parameters; the M-sized sums A A^T, A err and the scalars N, |y|^2 are all-reduced in the
# forward and the gradients in the backward, so every rank sees the bound and the gradients of the
# WHOLE data set (optimisers on all ranks stay in step).
SHARD_GROUP = None
BLOCKED_SOLVE_MIN_M = 2048   # from this many inducing points on, chunk right-solves go through the inverted 1024 x 1024 blocks
LANES = 2                # chunk pipelines in flight (1: strictly one chunk after the other)
SPLIT_K = 8              # partial accumulators of the A A^T accumulation (1: none)
SYRK_K_SLICE = 8192      # columns of a chunk per accumulation launch (0: the whole chunk at once)


def _all_reduce(t):
    import torch.distributed as dist
    if SHARD_GROUP is None:
        return t
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=None if SHARD_GROUP is True else SHARD_GROUP)
    return t


def _shard_rank():
    import torch.distributed as dist
    if SHARD_GROUP is None:
        return 0
    return dist.get_rank(None if SHARD_GROUP is True else SHARD_GROUP)


class _InducingPointsGP(GPModel):
    """sparse_gpr.py:22-73; default inducing points = k-means centres (util.py:34-49)."""

    def __init__(self, x, y, kernel, num_inducing_points=None, inducing_points=None, mean_function=None,
                 likelihood=None):
        super().__init__(x, y, kernel, likelihood, mean_function)
        if inducing_points is None:
            from scipy.cluster.vq import kmeans2
            if num_inducing_points is None:
                num_inducing_points = np.clip(x.shape[0] // 10, 1, 100)
            xn = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
            try:
                inducing_points = kmeans2(xn, int(num_inducing_points))[0]
            except np.linalg.LinAlgError:
                xp = xn + 1.0e-4 * xn.std(axis=0) * np.random.randn(*xn.shape)
                inducing_points = kmeans2(xp, int(num_inducing_points))[0]
        self.Z = Param(as_tensor(inducing_points))

    @property
    def num_inducing(self) -> int:
        return self.Z.shape[0]

    def _native_kernel(self):
        """the kernel if it is one of the native stationary kinds (fused assembly + native sweeps),
        else None (sums / products / Linear / static kernels: the kernel's own K and autograd)."""
        from .. import kernels
        k = self.kernel
        return k if isinstance(k, kernels.Stationary) and k._kind is not None else None

    def _kernel_adapter(self):
        """-> (make_asm, tensors): the kernel tensors an autograd node differentiates, and what builds the adapter from them
        inside the node (`make_asm(*tensors)`).  The ONE place the adapter is chosen: a native kind is differentiated w.r.t. its
        constrained variance and length-scales, any other kernel object w.r.t. its raw parameters."""
        k = self._native_kernel()
        if k is not None:
            return functools.partial(_NativeAsm, k._kind), [k.variance.transform(), k.length_scales.transform()]
        return functools.partial(_GenericAsm, self.kernel), [p for p in self.kernel.parameters() if p.requires_grad]

    def _data(self, x=None, y=None):
        """(x, y) of an evaluation: the model's own data where none is given."""
        x = x if x is not None else self.X
        y = y if y is not None else self.Y
        if not x.shape[0] == y.shape[0]:
            raise ValueError("X and Y must have same # data.")
        return x, y

    def _collapsed_predict(self, f_uu, fB, x_new, diag):
        """The predictive equations of a collapsed model (sparse_gpr.py:155-195) from its two factors, c^T in fB's extra rows:
        -> (tmp2^T c, var [ns, dy] or cov [ns, ns]) with tmp1^T = K(x*, Z) L^-T, tmp2^T = tmp1^T LB^-T and
        var = Kdiag(x*) - |tmp1|^2 + |tmp2|^2.  What turns tmp2^T c into the mean is the model's (VFE: / s2, FITC: + m(x*))."""
        kern = self.kernel
        ns, m, dy = x_new.shape[0], self.Z.shape[0], self.Y.shape[1]
        T1 = _ops.padded_like_factor(f_uu, ns)                                    # tmp1^T = K(x*, Z) L^-T
        T1[:ns, :m] = kern.K(x_new, self.Z.detach())
        f_uu.solve_right_lt(T1, ns)
        T2 = T1.clone()
        fB.solve_right_lt(T2, ns)                                                 # tmp2^T = tmp1^T LB^-T
        T2c = _ops.gemm_nt(T2, fB.A[m:], ns, dy, _ops.round_up(m, 16))            # tmp2^T c
        if diag:
            v = kern.Kdiag(x_new).detach() - _ops.row_sumsq(T1, ns, m) + _ops.row_sumsq(T2, ns, m)
            return T2c, v[:, None].expand_as(T2c)
        return T2c, _posterior_cov(kern.K(x_new), T2, T1, ns, m)


def _posterior_cov(Kss, G, A, ns, m):
    """K(x*) + G G^T - A A^T for [ns, m] factors G, A in zero-padded buffers (a fresh matrix: Kss is left as it is)."""
    kp = _ops.round_up(m, 16)
    cov = Kss.clone()
    _ops.gemm_nt(G, G, ns, ns, kp, alpha=1.0, beta=1.0, C=cov)
    _ops.gemm_nt(A, A, ns, ns, kp, alpha=-1.0, beta=1.0, C=cov)
    return cov


def _zeros(rows, cols, device):
    return torch.zeros(rows, cols, dtype=torch.float64, device=device)


def _chunks(n, nc):
    for c0 in range(0, n, nc):
        yield c0, min(nc, n - c0)


def _chunk_rows(n):
    """rows of x per streamed chunk of an n-row evaluation (forward and backward of VFE, SVGP and FITC alike)."""
    return min(_ops.round_up(n, _ops.LEAF), _ops.round_up(CHUNK_ROWS, _ops.LEAF))


def _blocked_solve(m, n):
    """whether a chunk's right-solve goes through the inverted 1024 x 1024 diagonal blocks of L_uu (see _stream_gram)."""
    return m >= BLOCKED_SOLVE_MIN_M and n >= 4 * m


def _solve_chunk(f_uu, wb_uu, At, Xo, r):
    """A_c^T = K(x_c, Z) L^-T for the r rows assembled in At -> the buffer that holds it: At itself (in place, the recursion down
    to the leaf inverses), or Xo when wb_uu = _ops.block_inverses(f_uu) is given (_blocked_solve).  The ONE place the choice is
    acted on: a backward that recomputes A_c^T (FITC) gets the forward's bits."""
    if wb_uu is None:
        return f_uu.solve_right_lt(At, r)
    m = f_uu.n
    _ops._native.check(_ops._native.lib().gpn_trsm_right_lt_blocked(_ops._stream(At.device), _ops._ptr(f_uu.A), m, f_uu.ld, _ops._ptr(wb_uu),
                                                                    _ops._ptr(At), r, At.stride(0), _ops._ptr(Xo), Xo.stride(0)),
                       "gpn_trsm_right_lt_blocked")
    return Xo


class _State:
    """what one evaluation of the bound leaves behind (all M-sized)."""
    __slots__ = ("f_uu", "fB", "AAT", "Aerr", "s2", "tr", "terms", "n", "n_all", "yy_all", "trkff")


class _NativeAsm:
    """K(x_c, Z), K(Z), Kdiag(x_c) and their gradient sweeps for a kernel with a native kind: the fused assembly
    kernel and the native sweeps (gpn_kernel_grad, gpn_kernel_grad_x2).  Built from the constrained (variance, length_scales);
    holds their detached values, and tensors() are the gradients w.r.t. these two, in this order and with their shapes."""

    def __init__(self, kind, var, ls):
        self.kind, self.var, self.ls = kind, var.detach(), ls.detach()

    def factor_uu(self, Z):
        return _ops.kernel_factor(self.kind, Z, self.var, self.ls, None)          # L = chol(K(Z)) (+ladder)

    def kuf(self, xc, Z, out, ldk):
        _ops.kernel_matrix(self.kind, xc, Z, self.var, self.ls, out=out, ldk=ldk)

    def trkff(self, x):
        return x.shape[0] * self.var[0]                                           # Kdiag = variance (kernels.py:174-179)

    def kdiag(self, xc):
        """-> (buffer, stride): Kdiag(x_c)[i] = buffer[i * stride]."""
        return self.var, 0                                                        # Kdiag = variance for every row

    # -- backward: accumulators for (variance, length_scales) and Z
    def begin(self, Z):
        self.g_var = torch.zeros(1, dtype=torch.float64, device=Z.device)
        self.g_ls = torch.zeros_like(self.ls)
        self.g_Z = torch.zeros_like(Z)

    def grad_uu(self, Z, Guu):
        gv, gl = _backward.kernel_backward(self.kind, Z, None, self.var, self.ls, Guu)
        self.g_var += gv
        self.g_ls += gl
        _backward.kernel_backward_x2(self.kind, Z, Z, self.var, self.ls, Guu, scale=2.0, out=self.g_Z)

    def grad_uf(self, xc, Z, G):
        gv, gl = _backward.kernel_backward(self.kind, xc, Z, self.var, self.ls, G)
        self.g_var += gv
        self.g_ls += gl
        _backward.kernel_backward_x2(self.kind, xc, Z, self.var, self.ls, G, out=self.g_Z)

    def grad_kdiag(self, xc, gv):
        self.g_var += gv.sum()

    def grad_trkff(self, x, coef, n_all):
        self.g_var += coef * n_all                                                 # d tr Kff / d variance = N

    def tensors(self):
        return [self.g_var, self.g_ls]


class _GenericAsm:
    """The same for ANY kernel object (sparse_gpr.py:126-129 takes whatever `self.kernel` is: sums,
    products, Linear, ...): K(x_c, Z) and K(Z) come from the kernel's own `K` (whose stationary
    leaves are the native assembly), and the gradient of sum(G * K) goes back through the kernel's own
    autograd nodes, chunk by chunk -- to the RAW parameters directly: built from those that require a gradient, and
    tensors() are the gradients w.r.t. them, in their order."""

    def __init__(self, kernel, *params):
        self.kernel, self.params = kernel, list(params)

    def factor_uu(self, Z):
        with torch.no_grad():
            return _ops.cholesky_factor(self.kernel.K(Z))

    def kuf(self, xc, Z, out, ldk):
        with torch.no_grad():
            out[:xc.shape[0], :Z.shape[0]] = self.kernel.K(xc, Z)

    def trkff(self, x):
        with torch.no_grad():
            return self.kernel.Kdiag(x).sum()

    def kdiag(self, xc):
        with torch.no_grad():
            return self.kernel.Kdiag(xc).contiguous(), 1

    def begin(self, Z):
        self.g_params = [torch.zeros_like(p) for p in self.params]
        self.g_Z = torch.zeros_like(Z)

    def _pull(self, out, G, Zg):
        grads = torch.autograd.grad(out, self.params + [Zg], grad_outputs=G, allow_unused=True)
        for acc, g in zip(self.g_params + [self.g_Z], grads):
            if g is not None:
                acc += g

    def grad_uu(self, Z, Guu):
        with torch.enable_grad():
            Zg = Z.detach().requires_grad_(True)
            self._pull(self.kernel.K(Zg), Guu, Zg)

    def grad_uf(self, xc, Z, G):
        with torch.enable_grad():
            Zg = Z.detach().requires_grad_(True)
            self._pull(self.kernel.K(xc, Zg), G, Zg)

    def grad_kdiag(self, xc, gv):
        with torch.enable_grad():
            s = (self.kernel.Kdiag(xc) * gv).sum()
            grads = torch.autograd.grad(s, self.params, allow_unused=True)
        for acc, g in zip(self.g_params, grads):
            if g is not None:
                acc += g

    def grad_trkff(self, x, coef, n_all):
        # row shards: every rank differentiates the diagonal of ITS rows; the all-reduce sums them
        with torch.enable_grad():
            tr = self.kernel.Kdiag(x).sum()
            grads = torch.autograd.grad(tr, self.params, allow_unused=True)
        for acc, g in zip(self.g_params, grads):
            if g is not None:
                acc += coef * g

    def tensors(self):
        return self.g_params


def _stream_gram(asm, x, err, Z, f_uu, fB, scale, rows_hook=None):
    """The N-sized part of a collapsed inducing-point likelihood, streamed over row chunks of x:
    -> (AAT = scale * sum_c A_c A_c^T in a buffer shaped like fB.A (lower), Aerr = sum_c A_c err_c [round_up(M, 16), dy]) with
    A_c^T = K(x_c, Z) L^-T.  rows_hook(buf, errT, ci, c0, r) (FITC): called on the chunk's stream between the right-solve and the
    transpose with the solved chunk buf [r, M]; it may rescale buf's rows in place and writes the chunk's residual operand
    errT [round_up(dy, 16), nc] itself (without a hook: err_c^T)."""
    dev = x.device
    n, dy = err.shape
    m = Z.shape[0]
    AAT = torch.zeros_like(fB.A)
    mp = _ops.round_up(m, 16)
    Aerr = _zeros(mp, dy, dev)
    nc = _chunk_rows(n)
    nchunks = (n + nc - 1) // nc
    # Two chunk pipelines on two streams: while one chunk's SYRK (whose 2080 tiles fill the
    # 1280 workgroup slots 1.6 times: a poor last round) accumulates, the next chunk's assembly,
    # right-solve and transpose already run next to it.  The accumulations into AAT / Aerr are
    # ordered by events.
    lanes = min(LANES, 2) if nchunks > 1 else 1
    cur = torch.cuda.current_stream(dev)
    streams = [cur] + [torch.cuda.Stream(device=dev) for _ in range(lanes - 1)]
    bufs = [(_zeros(nc + 16, f_uu.ld, dev), _zeros(mp, nc, dev), _zeros(_ops.round_up(dy, 16), nc, dev))
            for _ in range(lanes)]
    lib = _ops._native.lib()
    # round 4: the chunk's right-solve through the inverted 1024 x 1024 diagonal blocks of L_uu (gpn_trsm_right_lt_blocked:
    # M / 1024 steps of two large contractions) instead of the recursion down to the 128-wide leaf inverses, whose K <= 256
    # levels ran at ~12 TFLOP/s (round-3 review: colpanel_kernel 19 % of C5's kernel time); one more chunk-sized buffer per lane
    blocked = _blocked_solve(m, n)
    wb_uu = _ops.block_inverses(f_uu) if blocked else None
    xbufs = [_zeros(nc + 16, f_uu.ld, dev) for _ in range(lanes)] if blocked else None
    # split-K partial accumulators (see below): only when M^2/2 has too few 128x128 tiles to fill the GPU
    mt128 = (m + 127) // 128
    split = SPLIT_K if (mt128 * (mt128 + 1) // 2 < 4096 and nc >= 4096 * SPLIT_K) else 1
    parts = torch.zeros(split, AAT.shape[0], AAT.shape[1], dtype=torch.float64, device=dev) if split > 1 else None
    aerr_parts = torch.zeros(split, mp, dy, dtype=torch.float64, device=dev) if split > 1 else None
    acc_done = None                                                        # event: AAT/Aerr updated through chunk c-1
    # (the measured-and-off inverse form below produces A_c directly in the [M, rows] layout: there is no [rows, M] chunk for a row
    # hook to work on, so a hooked evaluation -- FITC -- never takes it, whatever INVERSE_MIN_M says)
    W_uu = _ops.lower_inverse(f_uu) if (rows_hook is None and m >= INVERSE_MIN_M and n >= 4 * m) else None
    for stq in streams[1:]:
        stq.wait_stream(cur)
    for ci, (c0, r) in enumerate(_chunks(n, nc)):
        stq = streams[ci % lanes]
        At, A, errT = bufs[ci % lanes]
        with torch.cuda.stream(stq):
            stream = _ops._stream(dev)
            if r < nc:                                                     # ragged tail: stale entries -> 0
                At.zero_(), A.zero_(), errT.zero_()
            asm.kuf(x[c0:c0 + r], Z, At, f_uu.ld)
            if W_uu is not None:
                # A_c = W Kuf_c, W = L^-1 lower triangular: block rows of INVERSE_BLOCK rows, each with the K range it
                # needs (k < its last row) as a plain contraction
                for b0 in range(0, m, INVERSE_BLOCK):
                    rows = min(INVERSE_BLOCK, m - b0)
                    _ops.gemm_nt(W_uu[b0:], At, rows, r, _ops.round_up(b0 + rows, 16), C=A[b0:])
            else:
                S = _solve_chunk(f_uu, wb_uu, At, xbufs[ci % lanes] if blocked else None, r)   # A_c^T = Kuf_c^T L^-T
                if rows_hook is not None:
                    rows_hook(S, errT, ci, c0, r)
                _ops._native.check(lib.gpn_transpose(stream, _ops._ptr(S), r, m, S.stride(0), _ops._ptr(A), nc), "gpn_transpose")
            if rows_hook is None:
                errT[:dy, :r] = err[c0:c0 + r].t()
            kp = _ops.round_up(r, 16)
            first = 0.0 if c0 == 0 else 1.0
            if acc_done is not None:
                stq.wait_event(acc_done)
            if split > 1 and kp % (16 * split) == 0:
                # split-K: M^2/2 alone is too few tiles for the GPU (M = 4096: 2080 64x64 tiles = 1.6
                # rounds of the 1280 slots, 528 128x128 tiles = 1.03 rounds of 512), so the chunk's K
                # range is dealt over `split` partial accumulators in ONE launch (8 x 528 tiles =
                # 8.25 rounds); the partials are summed once, after the last chunk
                _ops.gemm_nt_batched(A, A, m, m, kp // split, split, kp // split, kp // split, parts,
                                     alpha=scale, beta=first, lower=True)
                # A err likewise: a 4096 x 65536 matrix-vector product is 128 workgroups of 4096
                # K-steps each as one skinny contraction (0.98 ms), 8x more of 8x shorter ones here
                _ops.gemm_nt_batched(A, errT, m, dy, kp // split, split, kp // split, kp // split, aerr_parts, beta=first)
            else:
                # K slices in sequence: one launch over the whole chunk keeps every workgroup slot
                # for ~10 ms and the other lane's short kernels starve behind it (no pre-emption)
                ks = SYRK_K_SLICE or kp
                tgt = parts[0] if split > 1 else AAT
                for k0 in range(0, kp, ks):
                    kk = min(ks, kp - k0)
                    _ops.gemm_nt(A[:, k0:], A[:, k0:], m, m, kk, alpha=scale, beta=(first if k0 == 0 else 1.0), C=tgt, lower=True)
                _ops.gemm_nt(A, errT, m, dy, kp, beta=first, C=(aerr_parts[0] if split > 1 else Aerr))
            acc_done = torch.cuda.Event()
            acc_done.record(stq)
    for stq in streams[1:]:
        cur.wait_stream(stq)
    if acc_done is not None:
        cur.wait_event(acc_done)
    if split > 1:
        torch.sum(parts, dim=0, out=AAT)
        torch.sum(aerr_parts, dim=0, out=Aerr)
        del parts
    return AAT, Aerr


def _factor_B(fB, AAT, Aerr, m):
    """B = AAT + I = LB LB^T in fB (jitter ladder of functions.py:20-43), (Aerr)^T riding along as the factor's extra rows."""
    def attempt(jitter):
        fB.A.copy_(AAT)
        fB.A.diagonal()[:m].add_(1.0 if jitter is None else 1.0 + jitter)  # B = AAT + I
        fB.pack_rhs(Aerr)
        return fB.potrf()
    _ops._ladder(attempt)


def _vfe_forward(asm, x, err, Z, s2):
    """streamed evaluation of sparse_gpr.py:126-137 -> _State."""
    dev = x.device
    n, dy = err.shape
    m = Z.shape[0]
    st = _State()
    st.n, st.s2 = n, s2
    st.f_uu = f_uu = asm.factor_uu(Z)
    fB = _ops.Factor(m, dy, dev)
    st.AAT, Aerr = _stream_gram(asm, x, err, Z, f_uu, fB, 1.0 / s2)
    AAT = st.AAT
    # row shards: one all-reduce of the M-sized sums and of (N, |err|^2)
    scal = torch.tensor([float(n), 0.0, 0.0], dtype=torch.float64, device=dev)
    scal[1] = _ops.dot2d(err, err)
    scal[2] = asm.trkff(x)                                                 # tr Kff (sparse_gpr.py:139-141)
    if SHARD_GROUP is not None:
        _all_reduce(AAT)
        _all_reduce(Aerr)
        _all_reduce(scal)
    st.n_all, st.yy_all, st.trkff = int(round(scal[0].item())), scal[1], scal[2]
    st.Aerr = Aerr[:m]
    st.tr = _ops.diag_sum(AAT, m)
    _factor_B(fB, AAT, st.Aerr, m)
    st.fB = fB
    st.terms = fB.lml_terms()            # [sum log LB_ii, || LB^-1 A err ||^2 = s2^2 |c|^2, ...]
    return st


def _sandwich(U, W, m):
    """U W U^T for upper-triangular U = L^-T and dense symmetric W (zero-padded buffers)."""
    kp = _ops.round_up(m, 16)
    T = torch.zeros_like(U)
    _ops.gemm_nt(U, W, m, m, kp, C=T, tri=_ops.TRI_A_UPPER)              # T = U W   (W = W^T)
    R = torch.zeros_like(U)
    _ops.gemm_nt(T, U, m, m, kp, C=R, tri=_ops.TRI_B_UPPER)              # R = T U^T
    return R


def _factor_inverses(f_uu, fB, m):
    """what a collapsed backward starts from -> (U = L^-T, UB = LB^-T, B^-1 [m, m] symmetrised from its lower triangle)."""
    U = _backward._upper_inverse(f_uu)                                     # L^-T
    UB = _backward._upper_inverse(fB)                                      # LB^-T
    Binv = _backward._kinv_lower(fB, UB)[:m, :m]
    Binv = torch.tril(Binv) + torch.tril(Binv, -1).t()
    return U, UB, Binv


def _vfe_backward(asm, x, err, Z, st):
    """-> (dF/d noise [1] (constrained value), None: err is the data, sparse_gpr.py:125); the kernel / inducing-point
    gradients are left in `asm` (native kinds: w.r.t. the constrained variance / length-scales and Z; any other kernel:
    w.r.t. its raw parameters and Z)."""
    dev = x.device
    n, p = err.shape
    m, s = Z.shape[0], st.s2
    f_uu, fB = st.f_uu, st.fB
    mp, pp = _ops.round_up(m, 16), _ops.round_up(p, 16)
    U, UB, Binv = _factor_inverses(f_uu, fB, m)
    Bd = torch.tril(st.AAT[:m, :m]) + torch.tril(st.AAT[:m, :m], -1).t()
    Bd.diagonal().add_(1.0)
    eye = torch.eye(m, dtype=torch.float64, device=dev)
    # beta^T = c^T LB^-1: the extra rows hold (LB^-1 A err)^T = s c^T
    bt = _zeros(pp, f_uu.ld, dev)
    _ops.gemm_nt(fB.A[m:], UB, p, m, mp, alpha=1.0 / s, C=bt, tri=_ops.TRI_B_UPPER)
    beta = _zeros(mp, pp, dev)
    beta[:m, :p] = bt[:p, :m].t()
    bbT = _ops.gemm_nt(beta, beta, m, m, pp)
    W = torch.zeros_like(U)
    W[:m, :m] = p * (eye - Binv) - bbT
    P = _sandwich(U, W, m)                                                 # s * dF/dKuf = P Kuf + gamma err^T
    W[:m, :m] = 0.5 * p * (2.0 * eye - Binv - Bd) - 0.5 * bbT
    Guu = _sandwich(U, W, m)                                               # dF/dKuu
    gt = _ops.gemm_nt(bt, U, p, m, mp, tri=_ops.TRI_B_UPPER)              # gamma^T = beta^T L^-1

    # K(Z, Z) part (identical on every rank of a sharded run: counted on the first one only)
    asm.begin(Z)
    if _shard_rank() == 0:
        asm.grad_uu(Z, Guu[:m, :m])

    # K(x, Z) part, streamed:  G_c = 1/s [K(x_c, Z) | err_c] [P | gamma]^T
    ldk = mp + pp
    Bq = _zeros(mp, ldk, dev)
    Bq[:m, :m] = P[:m, :m]
    Bq[:m, mp:mp + p] = gt[:p, :m].t()
    nc = _chunk_rows(n)
    Kx = _zeros(nc + 16, ldk, dev)
    G = torch.empty(nc, mp, dtype=torch.float64, device=dev)
    for c0, r in _chunks(n, nc):
        xc = x[c0:c0 + r]
        asm.kuf(xc, Z, Kx, ldk)
        Kx[:r, mp:mp + p] = err[c0:c0 + r]
        _ops.gemm_nt(Kx, Bq, r, m, ldk, alpha=1.0 / s, C=G)
        asm.grad_uf(xc, Z, G[:r, :m])
    asm.grad_trkff(x, -0.5 * p / s, n if SHARD_GROUP is not None else st.n_all)   # -p/(2s) d tr Kff (this rank's rows)

    if SHARD_GROUP is not None:                                            # sum the row shards' contributions
        for t in asm.tensors() + [asm.g_Z]:
            _all_reduce(t)
    n_all = st.n_all
    c2 = st.terms[1] / (s * s)
    b = beta[:m, :p]
    quad = _ops.dot2d(b, st.Aerr) / s - _ops.dot2d(b, b)                   # beta^T (B - I) beta
    g_noise = (0.5 * p / s) * (m - _ops.diag_sum(Binv, m)) - c2 / s + 0.5 * quad / s - 0.5 * p * st.tr / s \
        - 0.5 * p * n_all / s + 0.5 * (st.yy_all + p * st.trkff) / (s * s)
    return g_noise.reshape(1), None


def _elbo(st, p, s2):
    """sparse_gpr.py:139-151 from the M-sized state."""
    n = st.n_all                                                           # N of the whole data set
    elbo = -0.5 * p * n * math.log(2.0 * math.pi)
    elbo = elbo - p * st.terms[0]
    elbo = elbo - 0.5 * p * n * math.log(s2)
    elbo = elbo - 0.5 * (st.yy_all + p * st.trkff) / s2
    elbo = elbo + 0.5 * st.terms[1] / (s2 * s2)                            # c = LB^-1 (A err) / s2
    elbo = elbo + 0.5 * p * st.tr
    return elbo


def _vfe_evaluate(asm, x, err, Z, noise):
    """-> (the bound, its state, the (x, err) its backward streams over).  The noise is read on the host once per evaluation;
    x and err are streamed as they come (row slices of either layout)."""
    s2 = float(noise.item())
    st = _vfe_forward(asm, x, err, Z, s2)
    return _elbo(st, err.shape[1], s2), st, x, err


class _CollapsedBound(torch.autograd.Function):
    """A collapsed inducing-point likelihood (VFE's bound, FITC's marginal likelihood) as one autograd node over
    (noise, Z, err, *kernel tensors of _InducingPointsGP._kernel_adapter).  The model brings
    evaluate(asm, x, err, Z, noise) -> (value, state, x, err) and backward(asm, x, err, Z, state) -> (dF/d noise, dF/d err or
    None) with the kernel / inducing-point gradients left in `asm`; the state is handed out through `holder`."""

    @staticmethod
    def forward(ctx, evaluate, backward, make_asm, holder, x, noise, Z, err, *tensors):
        ctx.asm, ctx.backward_fn = make_asm(*tensors), backward
        value, ctx.st, ctx.x, ctx.err = evaluate(ctx.asm, x, err, Z.detach(), noise)
        ctx.save_for_backward(Z)
        holder["state"] = ctx.st
        return value

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        Z, = ctx.saved_tensors
        g_noise, g_err = ctx.backward_fn(ctx.asm, ctx.x, ctx.err, Z.detach(), ctx.st)
        return (None, None, None, None, None, g * g_noise, g * ctx.asm.g_Z, g * g_err if ctx.needs_input_grad[7] else None) \
            + tuple(g * t for t in ctx.asm.tensors())


class VFE(_InducingPointsGP):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        assert isinstance(self.mean_function, Zero), "Mean functions not implemented for VFE yet."

    def _bound(self, x):
        holder = {}
        s2 = self.likelihood.variance.transform()
        make_asm, tensors = self._kernel_adapter()
        elbo = _CollapsedBound.apply(_vfe_evaluate, _vfe_backward, make_asm, holder, x, s2, self.Z,
                                     self.Y, *tensors)                   # sparse_gpr.py:125 quirk: err = self.Y
        return elbo, holder["state"]

    def log_likelihood(self, x=None, y=None):
        """variational lower bound, sparse_gpr.py:108-153 (0-dim tensor)."""
        return self._bound(self._data(x, y)[0])[0]

    def _state_for_predict(self, x):
        """the M-sized state of the bound (chol K(Z), chol B, c) that a prediction starts from.  The reference re-evaluates the bound
        inside every _predict (sparse_gpr.py:155-170: two factorisations and the N-sized solves again); here it is kept between
        predictions, like GPR's factor (GPModel._cached_state: the data by identity + version, every parameter -- inducing points
        included -- by value)."""
        return self._cached_state("vfe", x, lambda: self._bound(x)[1])

    def _predict(self, x_new, diag=True, x=None):
        """sparse_gpr.py:155-195."""
        x = x if x is not None else self.X
        with torch.no_grad():
            st = self._state_for_predict(x)
            T2c, cov = self._collapsed_predict(st.f_uu, st.fB, x_new, diag)
            return T2c / st.s2, cov                                                   # (the extra rows hold s2 c^T)


# =====================================================================================================================
# SVGP (sparse_gpr.py:198-381): minibatch bound, closed-form backward, prediction
# =====================================================================================================================
#
# With L = chol K(Z), alpha = K(x_b, Z) L^-T [nb, M], w = L^-1 m [M, dy], beta = L^-1 S_L [M, M], Q = beta beta^T - I:
#
#     f_mean0 = alpha w        f_var_i = Kdiag_i + alpha_i Q alpha_i^T        (sparse_gpr.py:367-377)
#     KL = dy/2 (|beta|_F^2 - M + 2 sum log L_ii - 2 sum log S_L,ii) + 1/2 |w|_F^2   (sum over output columns of the KL of
#                                                                                     sparse_gpr.py:293-306; the prior mean cancels)
#
# Backward for upstream (g_mean [nb, dy], g_var [nb], g_kl), with h = alpha^T g_mean and G_Q = alpha^T diag(g_var) alpha
# (accumulated over the row chunks) and U = L^-T:
#
#     G_alpha = g_mean w^T + 2 diag(g_var) alpha Q            dK(x_b, Z) = G_alpha U^T
#     G_w = h + g_kl w                                        d/dm   = U G_w
#     G_beta = 2 G_Q beta + g_kl dy beta                      d/dS_L = tril(U G_beta) - g_kl dy diag(1 / S_L,ii)
#     E = w h^T + h w^T + g_kl w w^T + 2 (Q G_Q + G_Q Q) + 2 G_Q + g_kl dy Q           (symmetric)
#     dK(Z, Z) = -1/2 U E U^T
#
# The last line is the sum of the three solves' pull-backs onto L (-L^-T [G_alpha^T alpha + G_w w^T + G_beta beta^T]) and of
# the log-determinant term (g_kl dy diag(1 / L_ii)) taken through the Cholesky pull-back L^-T Phi(L^T G_L) L^-1: the bracket
# is symmetric, so Phi (lower triangle, halved diagonal) and the symmetrisation collapse to the factor 1/2, and the
# log-determinant's share Phi(L^T diag(1 / L_ii)) = I / 2 turns the "+ g_kl dy (Q + I)" of G_beta beta^T into "+ g_kl dy Q".
# Checked against autograd through the reference's op chain by tests/golden/make_svgp_golden.py.
GAUSSIAN_SHORTCUT = True   # likelihoods.Gaussian: the data term without the sqrt / square round trip of propagate_log's Normal
# likelihoods.Bernoulli / Poisson / StudentT on the GPU: the data term and its gradients from ONE fused launch (csrc/lik.hip,
# gpn_lik_expect) instead of the torch ops of Likelihood.propagate_log on an [nb, H] tensor per column and their autograd twins
NATIVE_EXPECTATION = True


class _LikExpectNode(torch.autograd.Function):
    """The Gauss-Hermite expectation of a non-Gaussian log-likelihood as one autograd node over (f_mean [nb, dy], f_var [nb],
    y, *likelihood tensors): gpn_lik_expect once in the forward, which also leaves the gradients; the backward hands them back.
    `tensors`: () or, for Student-t, (scale^2 [1],) -- the constrained value, so the Param's transform is autograd's."""

    @staticmethod
    def forward(ctx, kind, df, H, f_mean, f_var, y, *tensors):
        dev = f_mean.device
        params = torch.cat([torch.full((1,), float(df), dtype=torch.float64, device=dev), tensors[0].detach().reshape(1)]) if tensors else None
        nodes, weights = (None, None) if kind == _ops._native.LIK_POISSON else _likelihood_rule(H, dev)
        value, g_mean, g_var, g_params = _ops.lik_expect(kind, params, f_mean.detach(), f_var.detach(), y.detach(), nodes, weights,
                                                         want_params=bool(tensors))
        ctx.save_for_backward(g_mean, g_var, g_params)
        ctx.shapes = [t.shape for t in tensors]
        return value

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        g_mean, g_var, g_params = ctx.saved_tensors
        return (None, None, None, g * g_mean, g * g_var, None) + tuple((g * g_params[1]).reshape(s) for s in ctx.shapes)


class _RobustMaxNode(torch.autograd.Function):
    """likelihoods.MultiClass.variational_expectation as one autograd node over (f_mean [nb, C], f_var [nb]):
    gpn_lik_expect_robustmax once in the forward (csrc/multiclass.hip), which also leaves the gradients."""

    @staticmethod
    def forward(ctx, eps, H, f_mean, f_var, labels):
        nodes, weights = _likelihood_rule(H, f_mean.device)
        value, g_mean, g_var = _ops.lik_expect_robustmax(f_mean.detach(), f_var.detach(), labels.detach(), eps, nodes, weights)
        ctx.save_for_backward(g_mean, g_var)
        return value

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        g_mean, g_var = ctx.saved_tensors
        return None, None, g * g_mean, g * g_var, None


def _likelihood_rule(H, device):
    from .. import likelihoods
    return likelihoods.gauss_hermite(H, device)


def _native_likelihood(lik):
    """-> (kind, df, tensors) of gpn_lik_expect for a likelihood whose type is EXACTLY one of the four native ones, else None
    (Gaussian, user likelihoods and subclasses -- which may override logp -- keep their propagate_log)."""
    from .. import likelihoods
    nat = _ops._native
    if type(lik) is likelihoods.Bernoulli:
        return (nat.LIK_PROBIT if lik.link == "probit" else nat.LIK_LOGIT), 0.0, ()
    if type(lik) is likelihoods.Poisson:
        return nat.LIK_POISSON, 0.0, ()
    if type(lik) is likelihoods.StudentT:
        s = lik.scale.transform()
        return nat.LIK_STUDENT_T, lik.df, (s * s,)
    return None


class _SVGPState:
    """the M-sized state of one evaluation (+ the single chunk's alpha and T, kept for the backward)."""
    __slots__ = ("f_uu", "betaT", "Q", "w", "kl", "saved", "nc")


def _sum_log_diag(A, m):
    out = torch.empty(3, dtype=torch.float64, device=A.device)
    _ops._native.check(_ops._native.lib().gpn_lml_reduce(_ops._stream(A.device), _ops._ptr(A), m, 0, A.stride(0), _ops._ptr(out)),
                       "gpn_lml_reduce")
    return out[0]


def _svgp_m_state(asm, Z, m_u, S_L):
    """chol K(Z), beta^T, Q, w and the KL term."""
    dev = Z.device
    m, dy = m_u.shape
    mp = _ops.round_up(m, 16)
    lib = _ops._native.lib()
    st = _SVGPState()
    st.f_uu = f_uu = asm.factor_uu(Z)
    ld = f_uu.ld
    st.betaT = BT = _ops.padded_like_factor(f_uu, m)                       # beta^T = S_L^T L^-T
    BT[:m, :m] = S_L.t()
    f_uu.solve_right_lt(BT, m)
    beta = _ops.zeros(BT.shape[0], ld, dev)
    _ops._native.check(lib.gpn_transpose(_ops._stream(dev), _ops._ptr(BT), m, m, ld, _ops._ptr(beta), ld), "gpn_transpose")
    st.Q = Q = _ops.zeros(BT.shape[0], ld, dev)
    _ops.gemm_nt(beta, beta, m, m, mp, C=Q)                                # beta beta^T
    bb = _ops.diag_sum(Q, m)                                               # |beta|_F^2 = tr(beta beta^T)
    Q.diagonal()[:m].sub_(1.0)
    WT = _ops.padded_like_factor(f_uu, dy)                                 # w^T = m^T L^-T
    WT[:dy, :m] = m_u.t()
    f_uu.solve_right_lt(WT, dy)
    st.w = w = WT[:dy, :m].t().contiguous()                                # [m, dy]
    S_c = _ops._c(S_L)
    st.kl = 0.5 * dy * (bb - m + 2.0 * f_uu.lml_terms()[0] - 2.0 * _sum_log_diag(S_c, m)) + 0.5 * _ops.dot2d(w, w)
    st.saved = None
    return st


def _svgp_alpha_T(asm, st, xc, Z, At, T):
    """alpha = K(x_c, Z) L^-T into At, T = alpha Q into T."""
    r, m = xc.shape[0], Z.shape[0]
    asm.kuf(xc, Z, At, st.f_uu.ld)
    st.f_uu.solve_right_lt(At, r)
    _ops.gemm_nt(At, st.Q, r, m, _ops.round_up(m, 16), C=T)


def _svgp_forward(asm, x, Z, m_u, S_L):
    """-> (f_mean0 [n, dy], f_var [n], state): sparse_gpr.py:358-377 without the mean function, rows streamed in chunks."""
    x = _ops._c(x)
    dev = x.device
    n, (m, dy) = x.shape[0], m_u.shape
    lib = _ops._native.lib()
    st = _svgp_m_state(asm, Z, m_u, S_L)
    ld = st.f_uu.ld
    st.nc = nc = _chunk_rows(n)
    f_mean = torch.empty(n, dy, dtype=torch.float64, device=dev)
    f_var = torch.empty(n, dtype=torch.float64, device=dev)
    At, T = _ops.zeros(nc + 16, ld, dev), _ops.zeros(nc, ld, dev)
    for c0, r in _chunks(n, nc):
        if c0 > 0 and r < nc:                                              # ragged tail of a multi-chunk evaluation: stale rows -> 0
            At.zero_()
        xc = x[c0:c0 + r]
        _svgp_alpha_T(asm, st, xc, Z, At, T)
        kd, kds = asm.kdiag(xc)
        _ops._native.check(lib.gpn_svgp_marginals(_ops._stream(dev), _ops._ptr(At), ld, _ops._ptr(T), ld, r, m, _ops._ptr(st.w), dy, dy,
                                                  _ops._ptr(kd), kds, _ops._ptr(f_mean[c0:]), _ops._ptr(f_var[c0:])),
                           "gpn_svgp_marginals")
    if n <= nc:
        st.saved = (At, T)                                                 # one chunk: the backward starts from these
    return f_mean, f_var, st


def _svgp_backward(asm, x, Z, S_L, st, g_mean, g_var, g_kl):
    """-> (d/d induced_output_mean [m, dy], d/d S_L [m, m]); kernel / inducing-point gradients are left in `asm`."""
    x = _ops._c(x)
    dev = x.device
    n, (m, dy) = x.shape[0], st.w.shape
    mp, dyp = _ops.round_up(m, 16), _ops.round_up(dy, 16)
    lib = _ops._native.lib()
    f_uu, w, Q, BT = st.f_uu, st.w, st.Q, st.betaT
    ld, nc = f_uu.ld, st.nc
    U = _backward._upper_inverse(f_uu)                                     # L^-T
    asm.begin(Z)
    GQ = _ops.zeros(Q.shape[0], ld, dev)
    h = _zeros(mp, dy, dev)
    aT, gaT = _ops.zeros(mp, nc, dev), _ops.zeros(mp, nc, dev)
    gmT = _zeros(dyp, nc, dev)
    Gx = torch.empty(nc, ld, dtype=torch.float64, device=dev)
    if st.saved is not None:
        At, T = st.saved
    else:
        At, T = _ops.zeros(nc + 16, ld, dev), _ops.zeros(nc, ld, dev)
    for c0, r in _chunks(n, nc):
        xc = x[c0:c0 + r]
        if st.saved is None:
            if c0 > 0 and r < nc:
                At.zero_(), gmT.zero_()
            _svgp_alpha_T(asm, st, xc, Z, At, T)
        gv, gm = _ops._c(g_var[c0:c0 + r]), _ops._c(g_mean[c0:c0 + r])
        _ops._native.check(lib.gpn_svgp_backward_rows(_ops._stream(dev), _ops._ptr(At), ld, _ops._ptr(T), ld, r, m, _ops._ptr(w), dy, dy,
                                                      _ops._ptr(gv), _ops._ptr(gm), _ops._ptr(aT), _ops._ptr(gaT), nc),
                           "gpn_svgp_backward_rows")
        gmT[:dy, :r] = gm.t()
        kp = _ops.round_up(r, 16)
        first = 0.0 if c0 == 0 else 1.0
        _ops.gemm_nt(gaT, aT, m, m, kp, beta=first, C=GQ)                  # G_Q += alpha^T diag(g_var) alpha
        _ops.gemm_nt(aT, gmT, m, dy, kp, beta=first, C=h)                  # h += alpha^T g_mean
        _ops.gemm_nt(T, U, r, m, mp, C=Gx, tri=_ops.TRI_B_UPPER)           # dK(x_c, Z) = G_alpha L^-1
        asm.grad_uf(xc, Z, Gx[:r, :m])
        asm.grad_kdiag(xc, gv)
    st.saved = None

    # M-sized part
    h = h[:m]
    GQs = torch.zeros_like(GQ)
    GQs[:m, :m] = 0.5 * (GQ[:m, :m] + GQ[:m, :m].t())                      # (symmetric up to the rounding of the two operands)
    QG = _ops.gemm_nt(Q, GQs, m, m, mp)                                    # Q G_Q
    kd = g_kl * dy
    E = _ops.matmul_nt(w, h)
    E = E + E.t() + g_kl * _ops.matmul_nt(w, w) + 2.0 * (QG + QG.t()) + 2.0 * GQs[:m, :m] + kd * Q[:m, :m]
    W = torch.zeros_like(U)
    W[:m, :m] = -0.5 * E
    asm.grad_uu(Z, _sandwich(U, W, m)[:m, :m])                             # dK(Z, Z) = -1/2 U E U^T
    GbT = torch.zeros_like(BT)
    _ops.gemm_nt(BT, GQs, m, m, mp, alpha=2.0, C=GbT)                      # G_beta^T = 2 beta^T G_Q + g_kl dy beta^T
    GbT[:m, :m] += kd * BT[:m, :m]
    g_S = torch.tril(_ops.gemm_nt(U, GbT, m, m, mp, tri=_ops.TRI_A_UPPER))  # L^-T G_beta, lower triangle
    g_S.diagonal().sub_(kd / S_L.diagonal())
    GwT = _zeros(dyp, ld, dev)
    GwT[:dy, :m] = (h + g_kl * w).t()
    g_m = _ops.gemm_nt(U, GwT, m, dy, mp, tri=_ops.TRI_A_UPPER)            # L^-T G_w
    return g_m, g_S


def _grads_or_zero(g_mean, g_var, g_kl, f_mean, f_var):
    g_mean = torch.zeros_like(f_mean) if g_mean is None else g_mean
    g_var = torch.zeros_like(f_var) if g_var is None else g_var
    g_kl = torch.zeros((), dtype=torch.float64, device=f_var.device) if g_kl is None else g_kl
    return g_mean, g_var, g_kl


class _SVGPNode(torch.autograd.Function):
    """q(f)'s marginals on a batch and KL(q(u) || p(u)) as one autograd node over (Z, induced_output_mean, S_L, *kernel tensors
    of _InducingPointsGP._kernel_adapter): -> (f_mean0 [nb, dy], f_var [nb], KL)."""

    @staticmethod
    def forward(ctx, make_asm, x, Z, m_u, S_L, *tensors):
        asm = make_asm(*tensors)
        f_mean, f_var, st = _svgp_forward(asm, x, Z.detach(), m_u.detach(), S_L.detach())
        ctx.asm, ctx.x, ctx.st = asm, x, st
        ctx.save_for_backward(Z, S_L, f_mean, f_var)
        return f_mean, f_var, st.kl

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_mean, g_var, g_kl):
        Z, S_L, f_mean, f_var = ctx.saved_tensors
        g_mean, g_var, g_kl = _grads_or_zero(g_mean, g_var, g_kl, f_mean, f_var)
        g_m, g_S = _svgp_backward(ctx.asm, ctx.x, Z.detach(), S_L.detach(), ctx.st, g_mean, g_var, g_kl)
        return (None, None, ctx.asm.g_Z, g_m, g_S) + tuple(ctx.asm.tensors())


# ---- host-side initialisation (sparse_gpr.py:310-335): runs once on <= 100 points, before the model moves to the GPU ------
def _host_K(kernel, X, X2=None):
    """K(X, X2) of the shell's kernel classes in plain fp64 torch on the host (the kernels' own `K` is native-only)."""
    from .. import kernels
    v = lambda p: p.transform().detach().cpu()
    other = X if X2 is None else X2
    if isinstance(kernel, kernels.Sum):
        return _host_K(kernel.kern1, X, X2) + _host_K(kernel.kern2, X, X2)
    if isinstance(kernel, kernels.Product):
        return _host_K(kernel.kern1, X, X2) * _host_K(kernel.kern2, X, X2)
    if isinstance(kernel, kernels.Linear):
        return (X * v(kernel.variance)) @ other.t()
    if isinstance(kernel, kernels.White):
        return v(kernel.variance).expand(X.shape[0]).diag() if X2 is None else torch.zeros(X.shape[0], other.shape[0], dtype=X.dtype)
    if isinstance(kernel, kernels.Constant):
        return v(kernel.variance).expand(X.shape[0], other.shape[0]).clone()
    if isinstance(kernel, kernels.Stationary) and kernel._kind is not None:
        ls, var = v(kernel.length_scales), v(kernel.variance)
        diff = (X / ls)[:, None, :] - (other / ls)[None, :, :]
        r2 = (diff * diff).sum(-1)
        kind = kernel._kind
        if kind == "Rbf":
            return var * torch.exp(-0.5 * r2)
        r = torch.sqrt(torch.clamp(r2, min=1e-40))
        if kind == "Matern52":
            return var * (1.0 + math.sqrt(5.0) * r + 5.0 / 3.0 * r2) * torch.exp(-math.sqrt(5.0) * r)
        if kind == "Matern32":
            return var * (1.0 + math.sqrt(3.0) * r) * torch.exp(-math.sqrt(3.0) * r)
        if kind == "Exp":
            return var * torch.exp(-r)
        if kind == "Periodic":
            return var * torch.cos(r)
    return kernel.K(X, X2).detach()                                        # a user's kernel: whatever its K does on the host


def _host_cholesky(A):
    """functions.cholesky on the host: plain try, then the jitter ladder of functions.py:20-43."""
    out = []

    def attempt(jitter):
        Aj = A if jitter is None else A + jitter * torch.eye(A.shape[0], dtype=A.dtype)
        L, info = torch.linalg.cholesky_ex(Aj)
        out[:] = [L]
        return int(info.item())
    _ops._ladder(attempt)
    return out[0]


class SVGP(_InducingPointsGP):
    """Sparse variational GP (Hensman et al. 2013 / 2015), sparse_gpr.py:219-381: q(u) = N(induced_output_mean + m(Z),
    S_L S_L^T) over the induced outputs, minibatches of `batch_size` rows per evaluation of the bound."""

    def __init__(self, x, y, kernel, num_inducing_points=None, inducing_points=None, mean_function=None, likelihood=None,
                 batch_size=None):
        from .. import likelihoods
        super().__init__(x, y, kernel, num_inducing_points=num_inducing_points, inducing_points=inducing_points,
                         mean_function=mean_function,
                         likelihood=likelihood if likelihood is not None else likelihoods.Gaussian())   # sparse_gpr.py:238
        self.batch_size = batch_size
        # a likelihood that couples the latent columns of a row (likelihoods.MultiClass) says how many there are; Y is then ONE
        # column of class labels, checked here once
        self._coupled = getattr(self.likelihood, "num_latent", None) is not None
        if self._coupled:
            self.likelihood.check_labels(self.Y)
        # (induced_output_mean does NOT include the mean function's contribution, sparse_gpr.py:257-261)
        self.induced_output_mean, self.induced_output_chol_cov = self._init_posterior()

    def _init_posterior(self):
        """sparse_gpr.py:310-335: the posterior at Z of an exact GP on <= 100 random points (one np.random.permutation draw)."""
        from .. import likelihoods
        from torch.distributions.transforms import LowerCholeskyTransform
        i = np.random.permutation(self.num_data)[0: min(self.num_data, 100)]
        with torch.no_grad():
            x, y = self.X[i].detach().cpu(), self.Y[i].detach().cpu()
            Z = self.Z.detach().cpu()
            if self._coupled:                                # regress on the one-hot targets: one latent column per class
                y = torch.nn.functional.one_hot(y[:, 0].long(), self.likelihood.num_latent).to(torch.float64)
            if isinstance(self.likelihood, likelihoods.Gaussian):
                s2 = self.likelihood.variance.transform().detach().cpu()
            else:
                s2 = torch.tensor([0.01 * y.numpy().var()], dtype=torch.float64)
            mean = lambda t: self.mean_function(t).detach().cpu()
            L = _host_cholesky(_host_K(self.kernel, x) + s2.expand(x.shape[0]).diag())                 # gpr.py:104
            A = torch.linalg.solve_triangular(L, _host_K(self.kernel, x, Z), upper=False)
            V = torch.linalg.solve_triangular(L, y - mean(x), upper=False)
            m_u = A.t() @ V                                                                           # gpr.py:107 minus m(Z) again
            cov = _host_K(self.kernel, Z) - A.t() @ A
            chol_cov = _host_cholesky(cov)
        dev = self.Z.device
        return Param(m_u.to(dev)), Param(chol_cov.to(dev), transform=LowerCholeskyTransform())

    def _marginals(self, x):
        """-> (f_mean0 [n, dy] without the mean function, f_var [n], KL) through the native node."""
        S_L = self.induced_output_chol_cov.transform()
        make_asm, tensors = self._kernel_adapter()
        return _SVGPNode.apply(make_asm, x, self.Z, self.induced_output_mean, S_L, *tensors)

    def _data_term(self, f_mean, f_var, y):
        """sum over output columns of likelihood.propagate_log(N(f_mean_j, f_var), y_j), sparse_gpr.py:276-283."""
        from .. import likelihoods
        lik = self.likelihood
        if GAUSSIAN_SHORTCUT and type(lik) is likelihoods.Gaussian:
            # likelihoods.py:125-144 summed over the columns, f_var used as it is
            s2 = lik.variance.transform()
            n = y.nelement()
            return (-0.5 * (n * (math.log(2.0 * math.pi) + torch.log(s2))
                            + (torch.sum((y - f_mean) ** 2) + y.shape[1] * f_var.sum()) / s2)).reshape(())
        if self._coupled:                                    # (MultiClass on the GPU: gpn_lik_expect_robustmax, under the same switch)
            return lik.variational_expectation(f_mean, f_var, y[:, 0]).reshape(())
        native = _native_likelihood(lik) if NATIVE_EXPECTATION and f_mean.is_cuda else None
        if native is not None:
            kind, df, tensors = native
            return _LikExpectNode.apply(kind, df, lik.num_gauss_hermite_points, f_mean, f_var, y, *tensors)
        sd = torch.sqrt(f_var)
        return torch.stack([lik.propagate_log(torch.distributions.Normal(f_mean[:, j], sd), y[:, j]).reshape(())
                            for j in range(y.shape[1])]).sum()

    def log_likelihood(self, x=None, y=None):
        """variational bound, sparse_gpr.py:198-216 (minibatch rule) and 263-308 (0-dim tensor)."""
        if x is not None:
            if y is None:                                                    # (the reference: `assert y is not None`)
                raise ValueError("y is required when x is given")
        elif self.batch_size is not None:
            i = np.random.permutation(self.num_data)[: self.batch_size]     # the reference's host draw, one per evaluation
            x, y = self.X[i, :], self.Y[i, :]
        else:
            x, y = self.X, self.Y
        x, y = self._data(x, y)
        f_mean0, f_var, kl = self._marginals(x)
        f_mean = f_mean0 + self.mean_function(x)
        return self._data_term(f_mean, f_var, y) * (self.num_data / x.shape[0]) - kl

    def _predict(self, x_new, diag=True, chol_kuu=None, **kwargs):
        """sparse_gpr.py:337-381; chol_kuu is accepted for the reference's signature (the factor is native here)."""
        with torch.no_grad():
            Z, m_u = self.Z.detach(), self.induced_output_mean.detach()
            S_L = self.induced_output_chol_cov.transform().detach()
            make_asm, tensors = self._kernel_adapter()
            asm = make_asm(*tensors)
            mu_x = self.mean_function(x_new)
            if diag:
                f_mean0, f_var, _ = _svgp_forward(asm, x_new, Z, m_u, S_L)
                f_mean = f_mean0 + mu_x
                return f_mean, f_var[:, None].expand_as(f_mean)
            st = _svgp_m_state(asm, Z, m_u, S_L)
            f_uu = st.f_uu
            ns, m, dy = x_new.shape[0], Z.shape[0], m_u.shape[1]
            kp = _ops.round_up(m, 16)
            At = _ops.padded_like_factor(f_uu, ns)
            asm.kuf(_ops._c(x_new), Z, At, f_uu.ld)
            f_uu.solve_right_lt(At, ns)                                                       # alpha
            Gm = _ops.padded_like_factor(f_uu, ns)
            _ops.gemm_nt(At, st.betaT, ns, m, kp, C=Gm)                                       # gamma = alpha beta
            wT = _zeros(_ops.round_up(dy, 16), f_uu.ld, x_new.device)
            wT[:dy, :m] = st.w.t()
            f_mean = _ops.gemm_nt(At, wT, ns, dy, kp) + mu_x
            return f_mean, _posterior_cov(self.kernel.K(x_new), Gm, At, ns, m)
