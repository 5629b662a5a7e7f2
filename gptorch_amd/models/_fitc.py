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

from .. import _ops
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


def _fitc_evaluate(asm, x, err, Z, noise):
    """-> (log p(Y), its state, the contiguous (x, err) the row kernels of forward and backward read) for the node
    (sparse_gpr._CollapsedBound).  The noise is read on the host once per evaluation."""
    s2 = float(noise.item())
    x, err = _ops._c(x), _ops._c(err.detach())
    st = _fitc_forward(asm, x, err, Z, s2)
    return _lml(st, err.shape[1]), st, x, err


def _fitc_backward(asm, x, err, Z, st):
    """-> (dF/d noise [1], dF/d err [N, dy]); the kernel / inducing-point gradients are left in `asm` (as sparse_gpr._vfe_backward)."""
    dev = x.device
    n, p = err.shape
    m = Z.shape[0]
    f_uu, fB, lam = st.f_uu, st.fB, st.lam
    ld = f_uu.ld
    mp, pp = _ops.round_up(m, 16), _ops.round_up(p, 16)
    lib = _ops._native.lib()
    U, UB, Binv = _sg._factor_inverses(f_uu, fB, m)
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
        asm.grad_kdiag(xc, 0.5 * g[c0:c0 + r])                             # dF/dKdiag_i = g_i / 2

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


class FITC(_sg._InducingPointsGP):
    """Fully independent training conditional sparse GP regression.  Any kernel object (native stationary kinds through the
    fused assembly and the native sweeps, everything else through the kernel's own K / Kdiag and autograd), any mean function,
    a Gaussian likelihood.  Not a VFE: multi_start_optimize runs FITC restarts one after the other."""

    def _bound(self, x, y):
        if _sg.SHARD_GROUP is not None:
            raise NotImplementedError("FITC does not shard rows over ranks (sparse_gpr.SHARD_GROUP is set)")
        holder = {}
        s2 = self.likelihood.variance.transform()
        err = y - self.mean_function(x)
        make_asm, tensors = self._kernel_adapter()
        lml = _sg._CollapsedBound.apply(_fitc_evaluate, _fitc_backward, make_asm, holder, x, s2, self.Z, err, *tensors)
        return lml, holder["state"]

    def log_likelihood(self, x=None, y=None):
        """log p(Y) under the FITC prior (0-dim tensor)."""
        return self._bound(*self._data(x, y))[0]

    def _state_for_predict(self, x):
        """chol K(Z), chol B and c, kept between predictions (GPModel._cached_state, as VFE._state_for_predict)."""
        return self._cached_state("fitc", x, lambda: self._bound(x, self.Y)[1])

    def _predict(self, x_new, diag=True, x=None):
        """The collapsed predictive equations (_InducingPointsGP._collapsed_predict) from FITC's state: mean = tmp2^T c + m(x*), var = Kdiag(x*) - |tmp1|^2 + |tmp2|^2 with
        tmp1^T = K(x*, Z) L^-T, tmp2^T = tmp1^T LB^-T."""
        x = x if x is not None else self.X
        with torch.no_grad():
            st = self._state_for_predict(x)
            T2c, cov = self._collapsed_predict(st.f_uu, st.fB, x_new, diag)
            return T2c + self.mean_function(x_new), cov
