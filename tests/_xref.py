"""
TEST INFRASTRUCTURE ONLY -- an extended-precision reference for the stationary kinds and for Sum / Product trees
over them, Linear, Constant / Bias and White.

The CPU oracle (oracle/gp_oracle.py) restates the reference's algorithm, Gram-trick distances included
(r^2 = |a|^2 + |b|^2 - 2 a.b, util.py:73-88 in the reference).  Next to a repeated point that leaves
rounding noise of order eps in r^2, i.e. sqrt(eps) in r, and Exp / Matern12 has a cusp at r = 0: the
oracle's own Exp values are only good to ~1e-7 there, far too coarse to judge a native kernel.

This module evaluates the same definitions without that noise and in numpy's long double (64-bit
mantissa on x86-64):
  - squared distances by direct differences, one coordinate at a time, with the reference's clamp
    r = sqrt(max(r^2, 1e-40)) and no gradient below it (kernels.py:161-172 in the reference);
  - K, Kdiag, Cholesky, triangular solves, GPR's LML (gpr.py:47-67), its closed-form gradients and
    predict_f / predict_y (gpr.py:88-117, base.py:348-360);
  - DirectGPR / DirectVFE: the fp64 oracles with only K replaced by direct differences, for autograd
    gradients w.r.t. points and for sizes beyond the long-double budget.

Tolerance rule (`tol`): a check of the native path is held to max(16 e64, floor), where e64 is the error
of a plain fp64 CPU evaluation (DirectGPR) of the same quantity against the long-double value.  This
scales each check with the conditioning of its problem; the floors (FLOOR) are at or below the suite's
GPR checks and an order of magnitude below the Gram-trick oracle's Exp errors.

gptorch_amd never imports this module.
"""
import math

import numpy as np
import torch

from oracle import gp_oracle as orc

LD = np.longdouble
CLAMP = 1e-40                      # kernels.py:172: r = sqrt(clamp(r^2, min=1e-40))
KINDS = ("Rbf", "Matern52", "Matern32", "Exp", "Matern12", "Periodic")
# tolerance floors: relative to max(1, |reference|) for the loss and the gradients, absolute for the
# rest (K entries and predictions are O(variance))
FLOOR = {"K": 1e-13, "dense_grad": 1e-11, "point_grad": 1e-11, "loss": 1e-10, "grad": 1e-9,
         "mean": 1e-10, "var": 1e-10}
SAFETY = 16.0

_S5 = np.sqrt(LD(5))
_S3 = np.sqrt(LD(3))


def ld(a):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=LD)


def rel_err(got, ref):
    """max |got - ref| / max(1, max |ref|), in long double."""
    got, ref = ld(got), ld(ref)
    return float(np.max(np.abs(got - ref)) / max(LD(1), np.max(np.abs(ref)) if ref.size else LD(1)))


def abs_err(got, ref):
    return float(np.max(np.abs(ld(got) - ld(ref)))) if np.size(ref) else 0.0


def tol(e64, what):
    return max(SAFETY * e64, FLOOR[what])


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
def _ls(length_scales, d):
    ls = np.atleast_1d(ld(length_scales))
    return ls if ls.size == d else np.full(d, ls[0], dtype=LD)


def scaled_sqdist(X, X2, length_scales):
    """r^2 [n, m] = sum_d ((x_d - x2_d) / ell_d)^2, one coordinate at a time (no n x m x d temporary)."""
    X = ld(X)
    X2 = X if X2 is None else ld(X2)
    ls = _ls(length_scales, X.shape[1])
    r2 = np.zeros((X.shape[0], X2.shape[0]), dtype=LD)
    for c in range(X.shape[1]):
        t = (X[:, c:c + 1] - X2[None, :, c]) / ls[c]
        r2 += t * t
    return r2


def k_of_r2(kind, r2, variance):
    """K and B = -(dK/dr) / r as functions of the scaled squared distance, so that
    dK/dlog(ell_d) = B s_d  (s_d = ((x_d - x2_d) / ell_d)^2)  and  dK/dx_d = -B (x_d - x2_d) / ell_d^2.
        Rbf       K = v exp(-r^2/2)                    B = K   (no clamp: r^2 enters directly)
        Matern52  K = v (1 + s5 r + 5/3 r^2) e^{-s5 r}  K' = -5/3 v r (1 + s5 r) e^{-s5 r}
        Matern32  K = v (1 + s3 r) e^{-s3 r}            K' = -3 v r e^{-s3 r}
        Exp       K = v e^{-r}                          K' = -v e^{-r}
        Periodic  K = v cos r                           K' = -v sin r
    B = 0 where r^2 < 1e-40: the clamp makes K constant there."""
    r2 = ld(r2)
    v = LD(variance)
    if kind == "Rbf":
        K = v * np.exp(-r2 / 2)
        return K, K.copy()
    dead = r2 < CLAMP
    r = np.sqrt(np.maximum(r2, LD(CLAMP)))
    if kind == "Matern52":
        e = np.exp(-_S5 * r)
        K = v * (1 + _S5 * r + LD(5) / 3 * r * r) * e
        B = v * LD(5) / 3 * (1 + _S5 * r) * e
    elif kind == "Matern32":
        e = np.exp(-_S3 * r)
        K = v * (1 + _S3 * r) * e
        B = 3 * v * e
    elif kind in ("Exp", "Matern12"):
        K = v * np.exp(-r)
        B = K / r
    elif kind == "Periodic":
        K = v * np.cos(r)
        B = v * np.sin(r) / r
    else:
        raise ValueError(kind)
    return K, np.where(dead, LD(0), B)


def K(kind, X, X2, variance, length_scales):
    return k_of_r2(kind, scaled_sqdist(X, X2, length_scales), variance)[0]


def Kdiag(X, variance):
    return np.full(np.shape(X)[0], LD(variance), dtype=LD)


def kernel_param_grads(kind, X, X2, variance, length_scales, W, ard, r2=None):
    """d sum(W * K(X, X2)) / d(log variance, log ell) -> (g_var [1], g_ls [d or 1]).  r2: scaled_sqdist(X, X2, length_scales) if the
    caller has it already."""
    X = ld(X)
    X2 = X if X2 is None else ld(X2)
    W = ld(W)
    ls = _ls(length_scales, X.shape[1])
    r2 = scaled_sqdist(X, X2, ls) if r2 is None else r2
    Km, B = k_of_r2(kind, r2, variance)
    WB = W * B
    if not ard:                                        # sum_d s_d = r^2: one pass instead of d
        return np.array([np.sum(W * Km)]), np.array([np.sum(WB * r2)])
    g = np.empty(X.shape[1], dtype=LD)
    for c in range(X.shape[1]):
        t = (X[:, c:c + 1] - X2[None, :, c]) / ls[c]
        g[c] = np.sum(WB * t * t)
    return np.array([np.sum(W * Km)]), g


def kernel_point_grads(kind, X, X2, variance, length_scales, W):
    """d sum(W * K(X, X2)) / dX and / dX2 (X2 = None: K(X), the gradient w.r.t. X through both arguments)."""
    X = ld(X)
    sym = X2 is None
    X2 = X if sym else ld(X2)
    W = ld(W)
    ls = _ls(length_scales, X.shape[1])
    WB = W * k_of_r2(kind, scaled_sqdist(X, X2, ls), variance)[1]
    gX = np.empty(X.shape, dtype=LD)
    gX2 = np.empty(X2.shape, dtype=LD)
    for c in range(X.shape[1]):
        t = (X[:, c:c + 1] - X2[None, :, c]) / (ls[c] * ls[c])
        gX[:, c] = -np.sum(WB * t, axis=1)
        gX2[:, c] = np.sum(WB * t, axis=0)
    return (gX + gX2) if sym else (gX, gX2)


# ---------------------------------------------------------------------------------------------------------------------
# expressions: Sum / Product trees (kernels.py:286-306) over stationary leaves, Linear (238-265), Constant / Bias (95-105)
# and White (83-92)
# ---------------------------------------------------------------------------------------------------------------------
# A spec is the tree in sum-of-products form: a list of groups, each a list of leaf dicts
#     {"id": key, "type": "stationary" | "linear" | "constant" | "white", "kind": one of KINDS (stationary only),
#      "variance": a number (linear: or one per input), "length_scales": a number or one per input (stationary only), "ard": bool}
# K = sum over groups of the elementwise product of the group's leaves.  Leaves with one id are ONE leaf (one set of
# parameters) standing in several groups, as in (a + b) * c = a c + b c.
def leaf(id, type, kind=None, variance=1.0, length_scales=None, ard=False):
    return {"id": id, "type": type, "kind": kind, "variance": variance, "length_scales": length_scales, "ard": ard}


def expand_tree(tree):
    """("+", a, b) / ("*", a, b) over leaf dicts -> spec, by distributivity (groups in the order a b-major expansion gives:
    (a + b) * (c + d) = a c + a d + b c + b d)."""
    if isinstance(tree, dict):
        return [[tree]]
    op, a, b = tree
    a, b = expand_tree(a), expand_tree(b)
    return a + b if op == "+" else [x + y for x in a for y in b]


def spec_leaves(spec):
    """the distinct leaves in first-visit order."""
    out = []
    for g in spec:
        for l in g:
            if all(l["id"] != q["id"] for q in out):
                out.append(l)
    return out


def split_instances(spec):
    """the same expression with every leaf instance a leaf of its own (ids (id, group, position)): its parameter gradients
    are the per-instance gradients of `spec`."""
    return [[dict(l, id=(l["id"], gi, ti)) for ti, l in enumerate(g)] for gi, g in enumerate(spec)]


def _lin_v(l, d):
    v = np.atleast_1d(ld(l["variance"]))
    return v if v.size == d else np.full(d, v[0], dtype=LD)


def leaf_K(l, X, X2, r2=None):
    """one leaf's K(X, X2) (X2 None: K(X)) in long double (r2: a stationary leaf's scaled_sqdist, if the caller has it)."""
    X = ld(X)
    sym = X2 is None
    X2 = X if sym else ld(X2)
    n, m = X.shape[0], X2.shape[0]
    t = l["type"]
    if t == "stationary":
        return k_of_r2(l["kind"], scaled_sqdist(X, X2, l["length_scales"]) if r2 is None else r2, l["variance"])[0]
    if t == "linear":
        return (X * _lin_v(l, X.shape[1])) @ X2.T
    if t == "constant":
        return np.full((n, m), LD(l["variance"]), dtype=LD)
    if t == "white":
        # kernels.py:83-92: the variance on the diagonal of K(X); identically zero for K(X, X2), whatever X2 holds
        return LD(l["variance"]) * np.eye(n, dtype=LD) if sym else np.zeros((n, m), dtype=LD)
    raise ValueError(t)


def leaf_Kdiag(l, X):
    X = ld(X)
    if l["type"] == "linear":
        return np.sum(X * X * _lin_v(l, X.shape[1]), 1)
    return np.full(X.shape[0], LD(l["variance"]), dtype=LD)      # kernels.py:67-80, 174-179 (White included)


def leaf_param_grads(l, X, X2, W, r2=None):
    """d sum(W * K_leaf(X, X2)) / d(log variance(s), log ell) -> (g_var, g_ls); g_ls is empty for a leaf without length scales."""
    X = ld(X)
    sym = X2 is None
    X2 = X if sym else ld(X2)
    W = ld(W)
    t = l["type"]
    none = np.zeros(0, dtype=LD)
    if t == "stationary":
        return kernel_param_grads(l["kind"], X, X2, l["variance"], l["length_scales"], W, l["ard"], r2=r2)
    if t == "linear":
        v = _lin_v(l, X.shape[1])
        g = np.array([v[c] * np.sum(W * np.outer(X[:, c], X2[:, c])) for c in range(X.shape[1])], dtype=LD)
        return (g if np.size(l["variance"]) > 1 or l["ard"] else np.array([g.sum()])), none
    if t == "constant":
        return np.array([LD(l["variance"]) * np.sum(W)]), none
    if t == "white":
        return np.array([LD(l["variance"]) * np.trace(W) if sym else LD(0)]), none
    raise ValueError(t)


def expr_K(spec, X, X2=None):
    """the long-double value of the expression."""
    total = None
    for g in spec:
        prod = None
        for l in g:
            Kl = leaf_K(l, X, X2)
            prod = Kl if prod is None else prod * Kl
        total = prod if total is None else total + prod
    return total


def expr_Kdiag(spec, X):
    total = None
    for g in spec:
        prod = None
        for l in g:
            Kl = leaf_Kdiag(l, X)
            prod = Kl if prod is None else prod * Kl
        total = prod if total is None else total + prod
    return total


def expr_param_grads(spec, X, X2, W, with_K=False):
    """d sum(W * K(X, X2)) / d log theta for every parameter of every distinct leaf, in closed form:
    {id: (g_var, g_ls)}.  A leaf instance sees the weight W * prod(other terms of its group); instances of one leaf add up.
    with_K: -> (gradients, expr_K(spec, X, X2)) from the same pass."""
    W = ld(W)
    out, total = {}, None
    for g in spec:
        r2s = [scaled_sqdist(X, X2, l["length_scales"]) if l["type"] == "stationary" else None for l in g]
        Ks = [leaf_K(l, X, X2, r2) for l, r2 in zip(g, r2s)]
        for ti, l in enumerate(g):
            Wt = W.copy()
            for ui, Ku in enumerate(Ks):
                if ui != ti:
                    Wt = Wt * Ku
            gv, gl = leaf_param_grads(l, X, X2, Wt, r2s[ti])
            if l["id"] in out:
                out[l["id"]] = (out[l["id"]][0] + gv, out[l["id"]][1] + gl)
            else:
                out[l["id"]] = (gv, gl)
        prod = Ks[0]
        for Ku in Ks[1:]:
            prod = prod * Ku
        total = prod if total is None else total + prod
    return (out, total) if with_K else out


def flat_grads(spec, grads):
    """{id: (g_var, g_ls)} -> the non-empty gradient vectors in leaf order (variance, then length scales)."""
    return [g for l in spec_leaves(spec) for g in grads[l["id"]] if np.size(g)]


# ---------------------------------------------------------------------------------------------------------------------
# dense linear algebra in long double
# ---------------------------------------------------------------------------------------------------------------------
_NB = 64


def cholesky(A):
    """lower L with L L^T = A (right-looking, 64-column panels); raises on a non-positive pivot."""
    A = np.array(ld(A), dtype=LD)
    n = A.shape[0]
    for k in range(0, n, _NB):
        e = min(k + _NB, n)
        for j in range(k, e):
            p = A[j, j]
            if not p > 0:
                raise np.linalg.LinAlgError("not positive definite at pivot %d (%r)" % (j, float(p)))
            A[j:, j] /= np.sqrt(p)
            A[j + 1:, j + 1:e] -= np.outer(A[j + 1:, j], A[j + 1:e, j])
        if e < n:
            P = A[e:, k:e]
            A[e:, e:] -= np.einsum("ik,jk->ij", P, P)
    return np.tril(A)


def solve_lower(L, B):
    """L^-1 B (forward substitution, 64-row blocks)."""
    X = np.array(ld(B), dtype=LD)
    vec = X.ndim == 1
    if vec:
        X = X[:, None]
    n = L.shape[0]
    for k in range(0, n, _NB):
        e = min(k + _NB, n)
        if k:
            X[k:e] -= np.einsum("ik,kj->ij", L[k:e, :k], X[:k])
        for i in range(k, e):
            if i > k:
                X[i] -= L[i, k:i] @ X[k:i]
            X[i] /= L[i, i]
    return X[:, 0] if vec else X


def solve_upper_t(L, B):
    """L^-T B (back substitution against the transposed lower factor)."""
    return solve_lower(L[::-1, ::-1].T, np.asarray(B)[::-1])[::-1]


# ---------------------------------------------------------------------------------------------------------------------
# GPR (gpr.py:47-117 of the reference) in long double
# ---------------------------------------------------------------------------------------------------------------------
class GPRRef:
    """Exact GPR with a stationary kernel or an expression, a Gaussian likelihood and a constant mean, every intermediate in long
    double.  Parameters are the constrained values; gradients are w.r.t. their logs (ExpTransform) and, for the mean,
    w.r.t. the value itself."""

    def __init__(self, x, y, kind, variance=None, length_scales=None, noise=None, ARD=False, mean=None):
        """kind: a stationary kind's name with (variance, length_scales, ARD) -- or an expression spec (expr_K), which carries its
        own parameters: GPRRef(x, y, spec, noise=..., mean=...)."""
        self.X, self.Y = ld(x), ld(y)
        self.n, self.dy = self.Y.shape
        self.noise = LD(noise)
        if isinstance(kind, str):
            self.spec = [[leaf("k", "stationary", kind, LD(variance), _ls(length_scales, self.X.shape[1]), ARD)]]
            self.kind, self.ARD, self.var, self.ls = kind, ARD, LD(variance), self.spec[0][0]["length_scales"]
        else:
            self.spec = kind
        self.mean = np.zeros(self.dy, dtype=LD) if mean is None else ld(mean)
        self.Kf = expr_K(self.spec, self.X, None)
        self.Kyy = self.Kf + self.noise * np.eye(self.n, dtype=LD)
        self.L = cholesky(self.Kyy)
        self.R = self.Y - self.mean
        self.alpha = solve_lower(self.L, self.R)

    def lml(self):
        return (-LD(0.5) * np.sum(self.alpha ** 2) - self.dy * np.sum(np.log(np.diag(self.L)))
                - LD(0.5) * self.dy * self.n * np.log(2 * LD(np.pi)))

    def loss(self):
        return -self.lml()

    def loss_grads(self):
        """d loss / d(log variance, log ell [d or 1], log noise, mean [dy]) -- for an expression: every distinct leaf's
        (log variance(s), log ell) in leaf order (flat_grads), then log noise and the mean -- with
        G = 1/2 (a a^T - dy Kyy^-1), a = Kyy^-1 (y - m):  dLML/dtheta = sum(G * dK/dtheta), dLML/dm = sum_i a_i."""
        a = solve_upper_t(self.L, self.alpha)
        Li = solve_lower(self.L, np.eye(self.n, dtype=LD))
        G = LD(0.5) * (a @ a.T - self.dy * np.einsum("ki,kj->ij", Li, Li))
        gk = flat_grads(self.spec, expr_param_grads(self.spec, self.X, None, G))
        g_noise = self.noise * np.trace(G)
        return [-g for g in gk] + [-np.array([g_noise]), -a.sum(0)]

    def predict_f(self, x_new, diag=True):
        xs = ld(x_new)
        A = solve_lower(self.L, expr_K(self.spec, self.X, xs))
        mean = A.T @ self.alpha + self.mean
        if diag:
            return mean, np.repeat((expr_Kdiag(self.spec, xs) - np.sum(A * A, 0))[:, None], self.dy, 1)
        return mean, expr_K(self.spec, xs, None) - A.T @ A

    def predict_y(self, x_new, diag=True):
        mean, v = self.predict_f(x_new, diag)
        return mean, (v + self.noise if diag else v + self.noise * np.eye(v.shape[0], dtype=LD))


# ---------------------------------------------------------------------------------------------------------------------
# fp64 oracles with direct-difference distances
# ---------------------------------------------------------------------------------------------------------------------
def direct_kernel_K(kind, X, X2, variance, length_scales):
    """oracle.kernel_K with r^2 by direct differences (differentiable w.r.t. everything, torch fp64)."""
    X2 = X if X2 is None else X2
    ls = length_scales.expand(X.shape[1])
    r2 = torch.zeros(X.shape[0], X2.shape[0], dtype=X.dtype)
    for c in range(X.shape[1]):
        t = (X[:, c:c + 1] - X2[:, c][None, :]) / ls[c]
        r2 = r2 + t * t
    if kind == "Rbf":
        return variance * torch.exp(-r2 / 2.0)
    r = torch.sqrt(torch.clamp(r2, min=CLAMP))
    if kind == "Matern52":
        s5 = math.sqrt(5.0)
        return variance * (1.0 + s5 * r + 5.0 / 3.0 * r * r) * torch.exp(-s5 * r)
    if kind == "Matern32":
        return variance * (1.0 + math.sqrt(3.0) * r) * torch.exp(-math.sqrt(3.0) * r)
    if kind in ("Exp", "Matern12"):
        return variance * torch.exp(-r)
    if kind == "Periodic":
        return variance * torch.cos(r)
    raise ValueError(kind)


def direct_expr_K(spec, X, X2=None, params=None):
    """expr_K in torch fp64 with direct_kernel_K for the stationary leaves -- the plain fp64 evaluation whose error against
    the long-double value is e64.  params: {id: (variance tensor, length-scale tensor or None)} (differentiable); default: the
    spec's own values as float64 tensors."""
    sym = X2 is None
    X2 = X if sym else X2
    n, m = X.shape[0], X2.shape[0]
    total = None
    for g in spec:
        prod = None
        for l in g:
            v, ls = params[l["id"]] if params is not None else leaf_tensors(l)
            t = l["type"]
            if t == "stationary":
                Kl = direct_kernel_K(l["kind"], X, X2, v, ls)
            elif t == "linear":
                Kl = (X * v) @ X2.t()
            elif t == "constant":
                Kl = v.expand(n, m)
            else:
                Kl = torch.diag(v.expand(n)) if sym else v * torch.zeros(n, m, dtype=X.dtype)
            prod = Kl if prod is None else prod * Kl
        total = prod if total is None else total + prod
    return total


def leaf_tensors(l, log=False, grad=False):
    """(variance, length scales or None) of a leaf as float64 tensors (their logs with log=True).  float64 explicitly:
    torch.tensor([0.8]) is float32 and would put 4e-8 into every "fp64" value."""
    def t(a):
        a = np.atleast_1d(np.asarray(a, dtype=np.float64))
        return torch.tensor(np.log(a) if log else a, dtype=torch.float64, requires_grad=grad)
    return t(l["variance"]), (None if l["length_scales"] is None else t(l["length_scales"]))


class DirectGPR(orc.GPROracle):
    """orc.GPROracle with K(X, X2) by direct differences (everything else: the reference's op chain in fp64).  kind: a stationary
    kind's name, or an expression spec (DirectGPR(x, y, kind=spec, noise=..., mean=...))."""

    def __init__(self, x, y, kind="Rbf", variance=1.0, length_scales=1.0, noise=None, ARD=False, mean=None):
        self.spec = None
        if isinstance(kind, str):
            super().__init__(x, y, kind=kind, variance=variance, length_scales=length_scales, noise=noise, ARD=ARD, mean=mean)
            return
        super().__init__(x, y, kind="Rbf", noise=noise, mean=mean)
        self.spec = kind
        self.raw = {l["id"]: leaf_tensors(l, log=True, grad=True) for l in spec_leaves(kind)}

    def parameters(self):
        """an expression: every distinct leaf's (raw variance(s), raw ell) in leaf order (GPRRef.loss_grads), then the raw noise"""
        if self.spec is None:
            return super().parameters()
        return [p for l in spec_leaves(self.spec) for p in self.raw[l["id"]] if p is not None] + [self.raw_noise]

    def K(self, X, X2=None):
        if self.spec is None:
            return direct_kernel_K(self.kind, X, X2, self.raw_variance.exp(), self.raw_length_scales.exp())
        return direct_expr_K(self.spec, X, X2, {i: (v.exp(), None if l is None else l.exp()) for i, (v, l) in self.raw.items()})

    def Kdiag(self, X):
        if self.spec is None:
            return orc.kernel_Kdiag(X, self.raw_variance.exp())
        total = 0.0
        for g in self.spec:
            prod = 1.0
            for l in g:
                v = self.raw[l["id"]][0].exp()
                prod = prod * ((X * X * v).sum(1) if l["type"] == "linear" else v.expand(X.shape[0]))
            total = total + prod
        return total

    def predict_f(self, x_new, diag=True):
        """gpr.py:88-117 (GPROracle.predict_f with this class's Kdiag)."""
        x_new = torch.as_tensor(np.asarray(x_new), dtype=orc.DTYPE)
        L = orc.cholesky(self.compute_kyy(self.X))
        A = orc.trtrs(self.K(self.X, x_new), L)
        V = orc.trtrs(self.Y - self._mean(self.X), L)
        mean_f = A.t() @ V + self._mean(x_new)
        if diag:
            return mean_f, (self.Kdiag(x_new) - (A * A).sum(0))[:, None].expand_as(mean_f)
        return mean_f, self.K(x_new) - A.t() @ A

    def loss_grads_with_mean(self):
        """loss and d loss / d(raw variance, raw ell, raw noise, mean) by autograd."""
        self.mean_val.requires_grad_(True)
        ps = self.parameters() + [self.mean_val]
        for p in ps:
            p.grad = None
        loss = self.loss()
        loss.backward()
        return loss.detach().clone(), [p.grad.detach().clone() for p in ps]


class DirectVFE(orc.VFEOracle):
    """orc.VFEOracle with K by direct differences."""

    def K(self, a, b=None):
        return direct_kernel_K(self.kind, a, b, self.variance, self.ls)
