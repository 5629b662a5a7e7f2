"""
FITC (Snelson & Ghahramani 2006): the third inducing-point model of gptorch/models/sparse_gpr.py (lines 76-90, an empty class
with a TODO in the reference).  The exact marginal likelihood of the prior whose covariance is Q = Kfu Kuu^-1 Kuf with the
DIAGONAL corrected to that of K:  err ~ N(0, Q + diag(Kdiag - diag Q) + s2 I)  per output column.

With L = chol K(Z), A = L^-1 K(Z, X) (M x N, column a_i), p = dy, err = Y - mean_function(X):

    lambda_i = Kdiag(x_i) - |a_i|^2 + s2,  D = diag(1 / lambda)
    B = I + A D A^T = LB LB^T,   b = A D err,   c = LB^-1 b
    F = -p N/2 log 2 pi - p/2 sum log lambda_i - p sum log LB_ii - 1/2 sum_i |err_i|^2 / lambda_i + 1/2 |c|_F^2

Forward.  VFE's streamed pipeline (sparse_gpr._stream_gram: two lanes, the blocked right-solve, split-K accumulation) with one
row kernel between a chunk's right-solve and its transpose (csrc/fitc.hip gpn_fitc_forward_rows: lambda, the rows scaled by
lambda^-1/2 in place, the scaled residual transposed, sum log lambda and sum err^2 / lambda), so that B is accumulated as the
GRAM form of the computed, scaled A D^1/2 with alpha = 1 -- positive semi-definite by construction, for the reason given at the
top of sparse_gpr.py.

Backward (closed form; tests/golden/make_fitc_golden.py checks it against autograd through the dense N x N form).  With
beta = B^-1 b, U = L^-T, r = D (err - A^T beta) (= Sigma^-1 err, N x p) and g_i = |r_i|^2 - p (1 / lambda_i - a_i^T B^-1 a_i / lambda_i^2):

    dF/dA   = beta r^T - p B^-1 A D - A diag(g)          (M x N, streamed per chunk: gpn_fitc_backward_rows)
    dF/dKuf = U dF/dA
    S       = (dF/dA) A^T = beta beta^T - p (I - B^-1) - A diag(g) A^T        dF/dKuu = -1/2 U S U^T
    dF/dKdiag_i = g_i / 2,   dF/ds2 = 1/2 sum g_i,   dF/derr = -r

Per chunk the backward recomputes alpha = A_c^T as the forward did, forms T = alpha [B^-1 | beta] in ONE dense contraction,
and the row kernel turns T into the rows of dF/dA^T and emits r, g and the transposed operands of A diag(g) A^T.
"""
import math

import torch

from .. import _backward, _ops
from . import sparse_gpr as _sg


class _FITCState:
    """what one evaluation leaves behind: the two factors (c^T in fB's extra rows), lambda [N] and the scalar sums."""
    __slots__ = ("f_uu", "fB", "s2", "lam", "sums", "terms", "n")


def _fitc_forward(asm, x, err, Z, s2):
    """streamed evaluation -> _FITCState (x [N, d], err [N, dy] contiguous)."""
    dev = x.device
    n, dy = err.shape
    m = Z.shape[0]
    lib = _ops._native.lib()
    st = _FITCState()
    st.n, st.s2 = n, s2
    st.f_uu = f_uu = asm.factor_uu(Z)
    fB = _ops.Factor(m, dy, dev)
    nc = _sg._chunk_rows(n)
    st.lam = lam = torch.empty(n, dtype=torch.float64, device=dev)
    sums = torch.zeros((n + nc - 1) // nc, 2, dtype=torch.float64, device=dev)              # per chunk: sum log lambda, sum err^2 / lambda
    work = [torch.empty(max(1, int(lib.gpn_fitc_forward_work_bytes(nc)) // 8), dtype=torch.float64, device=dev) for _ in range(2)]

    def rows(buf, errT, ci, c0, r):
        kd, kds = asm.kdiag(x[c0:c0 + r])
        _ops._native.check(lib.gpn_fitc_forward_rows(_ops._stream(dev), _ops._ptr(buf), buf.stride(0), r, m, _ops._ptr(err[c0:]), dy,
                                                     _ops._ptr(kd), kds, s2, _ops._ptr(errT), errT.stride(0), _ops._ptr(lam[c0:]),
                                                     _ops._ptr(work[ci % 2]), _ops._ptr(sums[ci])), "gpn_fitc_forward_rows")
    AAT, Aerr = _sg._stream_gram(asm, x, err, Z, f_uu, fB, 1.0, rows_hook=rows)              # A D A^T (Gram form), b = A D err
    _sg._factor_B(fB, AAT, Aerr[:m], m)
    st.fB = fB
    st.terms = fB.lml_terms()                                                              # [sum log LB_ii, |c|^2, ...]
    st.sums = torch.stack([_ops.dot2d(sums[:, 0:1]), _ops.dot2d(sums[:, 1:2])])
    return st


def _lml(st, p):
    return -0.5 * p * st.n * math.log(2.0 * math.pi) - 0.5 * p * st.sums[0] - p * st.terms[0] - 0.5 * st.sums[1] + 0.5 * st.terms[1]


def _fitc_backward(asm, x, err, Z, st):
    """-> (dF/d noise [1], dF/d err [N, dy]); the kernel / inducing-point gradients are left in `asm` (as sparse_gpr._vfe_backward)."""
    dev = x.device
    n, p = err.shape
    m = Z.shape[0]
    f_uu, fB, lam = st.f_uu, st.fB, st.lam
    ld = f_uu.ld
    mp, pp = _ops.round_up(m, 16), _ops.round_up(p, 16)
    lib = _ops._native.lib()
    U = _backward._upper_inverse(f_uu)                                     # L^-T
    UB = _backward._upper_inverse(fB)                                      # LB^-T
    Binv = _backward._kinv_lower(fB, UB)[:m, :m]
    Binv = torch.tril(Binv) + torch.tril(Binv, -1).t()
    bt = _ops.zeros(pp, ld, dev)                                           # beta^T = c^T LB^-1
    _ops.gemm_nt(fB.A[m:], UB, p, m, mp, C=bt, tri=_ops.TRI_B_UPPER)
    beta = bt[:p, :m].t().contiguous()                                     # [m, p]
    ldt = mp + pp
    Bq = _ops.zeros(ldt, mp, dev)                                          # [B^-1 | beta]^T: the chunk contraction's second operand
    Bq[:m, :m] = Binv
    Bq[mp:mp + p, :m] = bt[:p, :m]

    asm.begin(Z)
    nc = _sg._chunk_rows(n)
    wb_uu = _ops.block_inverses(f_uu) if _sg._blocked_solve(m, n) else None   # the forward's right-solve (_sg._solve_chunk)
    At = _ops.zeros(nc + 16, ld, dev)
    Xo = _ops.zeros(nc + 16, ld, dev) if wb_uu is not None else None
    T = torch.empty(nc, ldt, dtype=torch.float64, device=dev)
    aT, gaT = _ops.zeros(mp, nc, dev), _ops.zeros(mp, nc, dev)
    Gx = torch.empty(nc, ld, dtype=torch.float64, device=dev)
    AgA = _ops.zeros(U.shape[0], ld, dev)
    g = torch.empty(n, dtype=torch.float64, device=dev)
    r_all = torch.empty(n, p, dtype=torch.float64, device=dev)
    for c0, r in _sg._chunks(n, nc):
        xc = x[c0:c0 + r]
        if c0 > 0 and r < nc:                                              # ragged tail: stale rows -> 0
            At.zero_()
        asm.kuf(xc, Z, At, ld)
        stream = _ops._stream(dev)
        alpha = _sg._solve_chunk(f_uu, wb_uu, At, Xo, r)                   # alpha = K(x_c, Z) L^-T, as the forward formed it
        _ops.gemm_nt(alpha, Bq, r, mp + p, mp, C=T)                        # T = alpha [B^-1 | beta]
        _ops._native.check(lib.gpn_fitc_backward_rows(stream, _ops._ptr(alpha), alpha.stride(0), _ops._ptr(T), ldt, r, m, _ops._ptr(beta), p, p,
                                                      _ops._ptr(err[c0:]), _ops._ptr(lam[c0:]), _ops._ptr(r_all[c0:]), _ops._ptr(g[c0:]),
                                                      _ops._ptr(aT), _ops._ptr(gaT), nc), "gpn_fitc_backward_rows")
        kp = _ops.round_up(r, 16)
        _ops.gemm_nt(gaT, aT, m, m, kp, beta=(0.0 if c0 == 0 else 1.0), C=AgA)   # A diag(g) A^T
        _ops.gemm_nt(T, U, r, m, mp, C=Gx, tri=_ops.TRI_B_UPPER)           # dF/dK(x_c, Z) = (dF/dA^T) L^-1
        asm.grad_uf(xc, Z, Gx[:r, :m])
        asm.grad_kdiag(xc, 0.5 * g[c0:c0 + r])

    # K(Z, Z) part
    betap = _ops.zeros(mp, pp, dev)
    betap[:m, :p] = beta
    S = _ops.gemm_nt(betap, betap, m, m, pp)                               # beta beta^T
    S -= p * (torch.eye(m, dtype=torch.float64, device=dev) - Binv)
    S -= 0.5 * (AgA[:m, :m] + AgA[:m, :m].t())                             # (symmetric up to the rounding of the two operands)
    W = torch.zeros_like(U)
    W[:m, :m] = -0.5 * S
    asm.grad_uu(Z, _sg._sandwich(U, W, m)[:m, :m])                         # dF/dKuu = -1/2 U S U^T
    return (0.5 * g.sum()).reshape(1), r_all.neg_()


class _FITCBound(torch.autograd.Function):
    """The FITC marginal likelihood as one autograd node over (variance, length_scales, noise, Z, err)."""

    @staticmethod
    def forward(ctx, variance, length_scales, noise, Z, err, kind, x, holder):
        s2 = float(noise.item())
        asm = _sg._SVGPNativeAsm(kind, variance.detach(), length_scales.detach())
        x, err = _ops._c(x), _ops._c(err.detach())
        st = _fitc_forward(asm, x, err, Z.detach(), s2)
        ctx.asm, ctx.x, ctx.err, ctx.st = asm, x, err, st
        ctx.save_for_backward(length_scales, Z)
        holder["state"] = st
        return _lml(st, err.shape[1])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        length_scales, Z = ctx.saved_tensors
        g_noise, g_err = _fitc_backward(ctx.asm, ctx.x, ctx.err, Z.detach(), ctx.st)
        g_var, g_ls, g_Z = ctx.asm.tensors()
        g = grad_out
        return (g * g_var, g * g_ls.reshape(length_scales.shape), g * g_noise, g * g_Z,
                g * g_err if ctx.needs_input_grad[4] else None, None, None, None)


class _FITCBoundGeneric(torch.autograd.Function):
    """The same for any kernel object: node over (noise, Z, err, *raw kernel parameters); Kdiag(x_c) comes per chunk from the
    kernel, and its gradient is pulled with the weights g_c / 2."""

    @staticmethod
    def forward(ctx, noise, Z, err, kernel, x, holder, *params):
        s2 = float(noise.item())
        asm = _sg._SVGPGenericAsm(kernel, list(params))
        x, err = _ops._c(x), _ops._c(err.detach())
        st = _fitc_forward(asm, x, err, Z.detach(), s2)
        ctx.asm, ctx.x, ctx.err, ctx.st = asm, x, err, st
        ctx.save_for_backward(Z)
        holder["state"] = st
        return _lml(st, err.shape[1])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        Z, = ctx.saved_tensors
        g_noise, g_err = _fitc_backward(ctx.asm, ctx.x, ctx.err, Z.detach(), ctx.st)
        *g_params, g_Z = ctx.asm.tensors()
        g = grad_out
        return (g * g_noise, g * g_Z, g * g_err if ctx.needs_input_grad[2] else None, None, None, None) + tuple(g * t for t in g_params)


class FITC(_sg._InducingPointsGP):
    """Fully independent training conditional sparse GP regression.  Any kernel object (native stationary kinds through the
    fused assembly and the native sweeps, everything else through the kernel's own K / Kdiag and autograd), any mean function,
    a Gaussian likelihood.  Not a VFE: multi_start_optimize runs FITC restarts one after the other."""

    def _native_kernel(self):
        from .. import kernels
        k = self.kernel
        return k if isinstance(k, kernels.Stationary) and k._kind is not None else None

    def _bound(self, x, y):
        if _sg.SHARD_GROUP is not None:
            raise NotImplementedError("FITC does not shard rows over ranks (sparse_gpr.SHARD_GROUP is set)")
        k = self._native_kernel()
        holder = {}
        s2 = self.likelihood.variance.transform()
        err = y - self.mean_function(x)
        if k is not None:
            lml = _FITCBound.apply(k.variance.transform(), k.length_scales.transform(), s2, self.Z, err, k._kind, x, holder)
        else:
            params = [p for p in self.kernel.parameters() if p.requires_grad]
            lml = _FITCBoundGeneric.apply(s2, self.Z, err, self.kernel, x, holder, *params)
        return lml, holder["state"]

    def log_likelihood(self, x=None, y=None):
        """log p(Y) under the FITC prior (0-dim tensor)."""
        x = x if x is not None else self.X
        y = y if y is not None else self.Y
        if not x.shape[0] == y.shape[0]:
            raise ValueError("X and Y must have same # data.")
        return self._bound(x, y)[0]

    def _state_for_predict(self, x):
        """chol K(Z), chol B and c, kept between predictions (GPModel._cached_state, as VFE._state_for_predict)."""
        return self._cached_state("fitc", x, lambda: self._bound(x, self.Y)[1])

    def _predict(self, x_new, diag=True, x=None):
        """VFE's predictive equations from FITC's state: mean = tmp2^T c + m(x*), var = Kdiag(x*) - |tmp1|^2 + |tmp2|^2 with
        tmp1^T = K(x*, Z) L^-T, tmp2^T = tmp1^T LB^-T."""
        x = x if x is not None else self.X
        kern = self.kernel
        with torch.no_grad():
            st = self._state_for_predict(x)
            f_uu, fB = st.f_uu, st.fB
            ns, m, dy = x_new.shape[0], self.Z.shape[0], self.Y.shape[1]
            T1 = _ops.padded_like_factor(f_uu, ns)
            T1[:ns, :m] = kern.K(x_new, self.Z.detach())
            f_uu.solve_right_lt(T1, ns)
            T2 = T1.clone()
            fB.solve_right_lt(T2, ns)
            kp = _ops.round_up(m, 16)
            mean = _ops.gemm_nt(T2, fB.A[m:], ns, dy, kp) + self.mean_function(x_new)
            if diag:
                v = kern.Kdiag(x_new).detach() - _ops.row_sumsq(T1, ns, m) + _ops.row_sumsq(T2, ns, m)
                return mean, v[:, None].expand_as(mean)
            cov = kern.K(x_new).clone()
            _ops.gemm_nt(T2, T2, ns, ns, kp, alpha=1.0, beta=1.0, C=cov)
            _ops.gemm_nt(T1, T1, ns, ns, kp, alpha=-1.0, beta=1.0, C=cov)
        return mean, cov
