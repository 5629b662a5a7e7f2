"""The fused composite-kernel path (csrc/kexpr.hip: assembly, per-leaf gradient sweeps, the lock-step forms, the refinement's
residual pass) against the extended-precision reference of tests/_xref.py -- Sum / Product trees over every stationary kind,
Linear, Constant / Bias and White, at the shapes where kexpr.hip changes path (16 coordinates staged per pass, ARD gradients out
of the staged chunk at d <= 16, programs of 16 terms / 8 groups) and on points with the kernels' edges planted (repeated rows,
rows under and just above the clamp, a far row, Periodic's sign changes, X2 sharing rows with X).

Every numeric check is held to xr.tol: 16 x the error of a plain fp64 CPU evaluation of the same quantity (xr.direct_expr_K:
direct-difference distances) against the long-double value, floored (tests/_xref.py FLOOR).  Each check prints its figures
(`xref <family> <what> err e64 tol`) before it asserts.

gptorch_amd.kernels.Linear always carries one variance per input, so through Kernel.K a Linear leaf has ONE variance only at
d = 1; the one-variance sweep with its chunked staging (d > 16) is driven through the ABI with a hand-built term table."""
import ctypes
import math

import numpy as np
import pytest
import torch

from gptorch_amd import _native, _ops, kernels, likelihoods, mean_functions, rng
from gptorch_amd.models import GPR
from tests import _xref as xr
from tests.test_gpu_kinds_xref import KERN, _points

pytestmark = pytest.mark.gpu
LD = xr.LD


def _t(a, device=None, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=device, requires_grad=grad)


def _hold(family, what, err, e64, floor):
    """print the figures, then assert err <= xr.tol(e64, floor)."""
    tol = xr.tol(e64, floor)
    print("xref %s %s err=%.3e e64=%.3e tol=%.3e" % (family, what, err, e64, tol))
    assert err <= tol, (family, what, err, e64, tol)


# ---- trees ------------------------------------------------------------------------------------------------------------------
def st(id, kind, var, rel, d, ard=False):
    """a stationary leaf; length scale(s) rel x sqrt(d), ARD: spread over 0.6 .. 1.4 of that."""
    base = rel * math.sqrt(d)
    ls = base * (0.6 + 0.8 * rng.uniform(len(id) + 31 * d, d)) if ard else float(base)
    return xr.leaf(id, "stationary", kind, float(var), ls, ard)


def lin(id, d, lo=0.3, hi=0.9):
    """Linear as the package holds it: one variance per input (d = 1: one variance)."""
    return xr.leaf(id, "linear", variance=np.linspace(lo, hi, d) / math.sqrt(d), ard=True)


def const(id, var, bias=False):
    return dict(xr.leaf(id, "constant", variance=float(var)), bias=bias)


def white(id, var):
    return xr.leaf(id, "white", variance=float(var))


def _fold(op, leaves):
    tree = leaves[0]
    for l in leaves[1:]:
        tree = (op, tree, l)
    return tree


def _many(k, d, var=1.0, rel=2.5):
    """k isotropic stationary leaves cycling through the kinds.  Defaults: long length scales and variances near 1, so that a
    product of all of them stays O(1); a sum takes small variances and ordinary length scales."""
    return [st("k%d" % i, xr.KINDS[i % 6], var * (1.0 + 0.01 * i), rel + 0.1 * i, d) for i in range(k)]


# name -> (tree(d), fused_program() exists)
TREES = {
    "rbf*m52": (lambda d: ("*", st("rbf", "Rbf", 1.3, 0.8, d), st("m52", "Matern52", 0.9, 1.1, d)), True),
    "m32*exp": (lambda d: ("*", st("m32", "Matern32", 0.6, 0.9, d), st("exp", "Exp", 1.3, 1.2, d)), True),
    "m12*per": (lambda d: ("*", st("m12", "Matern12", 1.1, 1.0, d), st("per", "Periodic", 0.8, 0.8, d)), True),
    "ard_pairs": (lambda d: ("+", ("+", ("*", st("rbf", "Rbf", 1.3, 0.8, d, True), st("per", "Periodic", 0.8, 0.9, d, True)),
                                   ("*", st("m52", "Matern52", 0.9, 1.1, d, True), st("exp", "Exp", 1.3, 1.2, d, True))),
                             ("*", st("m32", "Matern32", 0.6, 0.9, d, True), st("m12", "Matern12", 1.1, 1.0, d, True))), True),
    "lin+rbf+const": (lambda d: ("+", ("+", lin("lin", d), st("rbf", "Rbf", 1.2, 0.8, d)), const("c", 0.4)), True),
    "lin*m52+bias": (lambda d: ("+", ("*", lin("lin", d), st("m52", "Matern52", 1.4, 0.9, d)), const("b", 0.2, bias=True)), True),
    "m52+white": (lambda d: ("+", st("m52", "Matern52", 0.9, 0.8, d), white("wh", 0.3)), True),
    "(m32+white)*rbf_ard": (lambda d: ("*", ("+", st("m32", "Matern32", 0.9, 1.0, d), white("wh", 0.3)), st("rbf", "Rbf", 1.1, 0.8, d, True)), True),
    "white*exp": (lambda d: ("*", white("wh", 0.3), st("exp", "Exp", 1.3, 0.8, d)), True),
    "(a+b)*(c+d)": (lambda d: ("*", ("+", st("rbf", "Rbf", 0.7, 0.8, d), const("b", 0.2, bias=True)),
                               ("+", st("m52", "Matern52", 1.4, 0.9, d), lin("lin", d))), True),
    "prod16": (lambda d: _fold("*", _many(16, d)), True),                                            # 16 terms in one group
    "sum8*lin": (lambda d: ("*", _fold("+", _many(8, d, 0.15, 0.8)), lin("lin", d)), True),                      # 8 groups, 16 terms
    "prod17": (lambda d: _fold("*", _many(17, d)), False),                                           # over GPN_EXPR_MAX_TERMS
    "sum9*const": (lambda d: ("*", _fold("+", _many(9, d, 0.15, 0.8)), const("c", 0.4)), False),                 # over GPN_EXPR_MAX_GROUPS
}
CLAMP_TREES = ("rbf*m52", "m32*exp", "m12*per")       # exact zero length-scale gradients under the clamp, leaf by leaf


def _package(tree, d, objs):
    """the package's kernel of a tree; leaves with one id become ONE object (objs: id -> leaf kernel)."""
    if not isinstance(tree, dict):
        op, a, b = tree
        a, b = _package(a, d, objs), _package(b, d, objs)
        return a + b if op == "+" else a * b
    l = tree
    if l["id"] not in objs:
        if l["type"] == "stationary":
            ls = np.asarray(l["length_scales"], dtype=np.float64) if l["ard"] else float(l["length_scales"])
            k = KERN[l["kind"]](d, variance=l["variance"], length_scales=ls, ARD=l["ard"])
        elif l["type"] == "linear":
            k = kernels.Linear(d, variance=np.asarray(l["variance"], dtype=np.float64))
        elif l["type"] == "white":
            k = kernels.White(d, variance=l["variance"])
        else:
            k = (kernels.Bias if l.get("bias") else kernels.Constant)(d, variance=l["variance"])
        objs[l["id"]] = k
    return objs[l["id"]]


def _raw_grads(spec, objs):
    """.grad of every raw (log) parameter in the order of xr.flat_grads"""
    out = []
    for l in xr.spec_leaves(spec):
        ps = [objs[l["id"]].variance] + ([objs[l["id"]].length_scales] if l["type"] == "stationary" else [])
        out += [torch.zeros_like(q) if q.grad is None else q.grad for q in ps]      # composed path: no node, no gradient (White in K(X, X2))
    return out


def _direct64(spec, xn, x2n, wn):
    """fp64 CPU evaluation by direct differences: K and d sum(W K)/d(log theta) by autograd, in the order of xr.flat_grads."""
    raw = {l["id"]: xr.leaf_tensors(l, log=True, grad=True) for l in xr.spec_leaves(spec)}
    Kd = xr.direct_expr_K(spec, _t(xn), None if x2n is None else _t(x2n), {i: (v.exp(), None if s is None else s.exp()) for i, (v, s) in raw.items()})
    (Kd * _t(wn)).sum().backward()
    zero = lambda p: torch.zeros_like(p) if p.grad is None else p.grad
    return Kd.detach(), [zero(p) for l in xr.spec_leaves(spec) for p in raw[l["id"]] if p is not None]


def _ls0(spec):
    """the length scale the edges are planted against: the tree's Periodic leaf, else its first stationary leaf"""
    sta = [l for l in xr.spec_leaves(spec) if l["type"] == "stationary"]
    pick = next((l for l in sta if l["kind"] == "Periodic"), sta[0])
    return float(np.atleast_1d(pick["length_scales"])[0])


def _planted(spec, seed, n, d, first=0):
    """test_gpu_kinds_xref._points; with a Linear leaf the far row sits at 40 ell, not 1000 (one Linear entry of ~1e6 would set the
    scale of the whole comparison)."""
    ls0 = _ls0(spec)
    x = _points(seed, n, d, ls0, first=first)
    if any(l["type"] == "linear" for l in xr.spec_leaves(spec)) and first + 28 < n:
        x[first + 28] = 0.0
        x[first + 28, 0] = 40.0 * ls0
    return x


def _max_err(gots, refs):
    return max(xr.rel_err(g.detach().cpu() if isinstance(g, torch.Tensor) else g, r) for g, r in zip(gots, refs))


# ---- (a) assembly and dense-mode sweeps through Kernel.K --------------------------------------------------------------------
SHAPES = [(1, 1, 1), (63, 65, 15), (64, 64, 16), (65, 63, 17), (129, 128, 32), (128, 129, 33), (130, 257, 48)]


@pytest.mark.parametrize("name", list(TREES))
@pytest.mark.parametrize("n,m,d", SHAPES)
def test_expression_matrix_and_dense_gradients(device, name, n, m, d):
    """Kernel.K(X), K(X, X2) of a Sum / Product tree (gpn_kernel_matrix_expr) and d sum(W K)/d(raw parameter) (gpn_kernel_expr_grad,
    dense mode, one sweep per leaf instance) against xr.expr_K / xr.expr_param_grads.  The fused node runs wherever
    prog.grad_supported(d) holds; per-input parameters at d > 16 and trees over the program limits take the composed path and meet
    the same tolerance."""
    make, has_prog = TREES[name]
    tree = make(d)
    spec = xr.expand_tree(tree)
    objs = {}
    k = _package(tree, d, objs)
    k.cuda()
    xn = _planted(spec, n + 7 * d, n, d)
    x2n = _planted(spec, m + 11 * d, m, d, first=3)
    k2 = min(n, len(range(1, m, 5)))
    x2n[1:5 * k2:5] = xn[:k2]
    X, X2 = _t(xn, device), _t(x2n, device)
    prog = k.fused_program()
    assert (prog is not None) == has_prog
    if name == "prod16":
        assert len(prog.instances) == _native.EXPR_MAX_TERMS and prog.ngroups == 1
    if name == "sum8*lin":
        assert len(prog.instances) == _native.EXPR_MAX_TERMS and prog.ngroups == _native.EXPR_MAX_GROUPS
    fused = prog is not None and prog.grad_supported(d)
    linear = any(l["type"] == "linear" for l in xr.spec_leaves(spec))
    for other, wseed in ((None, 1), (x2n, 2)):
        wn = rng.normal(100 * d + n + wseed, (n, n if other is None else m))
        k.zero_grad()
        Kg = k.K(X, None if other is None else X2)
        assert (type(Kg.grad_fn).__name__ == "ExprKBackward") == fused, type(Kg.grad_fn).__name__
        (Kg * _t(wn, device)).sum().backward()
        gr, Kr = xr.expr_param_grads(spec, xn, other, wn, with_K=True)
        gr = xr.flat_grads(spec, gr)
        K64, g64 = _direct64(spec, xn, other, wn)
        Kg = Kg.detach().cpu()
        _hold("a", "K", xr.rel_err(Kg, Kr), xr.rel_err(K64, Kr), "K")
        _hold("a", "grad", _max_err(_raw_grads(spec, objs), gr), _max_err(g64, gr), "dense_grad")
        if other is None and not linear:
            assert torch.equal(Kg, Kg.t())
        if other is not None and name == "white*exp":
            assert torch.count_nonzero(Kg) == 0            # a group with White: exactly 0 across two sets, shared rows included
    if name in CLAMP_TREES:
        # weights only on pairs under a leaf's clamp (Rbf: on exact repeats): its length-scale gradient is exactly 0
        wn = rng.normal(300 + d + n, (n, n))
        for l in xr.spec_leaves(spec):
            r2 = xr.scaled_sqdist(xn, None, l["length_scales"])
            wz = np.where(r2 == 0 if l["kind"] == "Rbf" else r2 < xr.CLAMP, wn, 0.0)
            assert np.count_nonzero(wz) > n or n < 8            # the planted pairs, not just the diagonal
            k.zero_grad()
            (k.K(X) * _t(wz, device)).sum().backward()
            assert torch.count_nonzero(objs[l["id"]].length_scales.grad) == 0
            gr = xr.expr_param_grads(spec, xn, None, wz)[l["id"]][0]
            g64 = _direct64(spec, xn, None, wz)[1]
            i64 = [q["id"] for q in xr.spec_leaves(spec) for _ in range(2)].index(l["id"])
            _hold("a", "clamp_var", xr.rel_err(objs[l["id"]].variance.grad.cpu(), gr), xr.rel_err(g64[i64], gr), "dense_grad")


# ---- (b) the ABI directly ---------------------------------------------------------------------------------------------------
_TYPE = {"stationary": _native.TERM_STATIONARY, "linear": _native.TERM_LINEAR, "constant": _native.TERM_CONSTANT, "white": _native.TERM_WHITE}


class _Prog:
    """a term table (include/gpnative.h gpn_expr_term) built from a spec by hand, theta packed leaf by leaf (variance(s), then
    length scale(s)); off[id] = (var_off, nvar, ls_off, nls)."""

    def __init__(self, spec):
        self.spec, self.off, theta = spec, {}, []
        for l in xr.spec_leaves(spec):
            v = np.atleast_1d(np.asarray(l["variance"], dtype=np.float64))
            s = np.zeros(0) if l["length_scales"] is None else np.atleast_1d(np.asarray(l["length_scales"], dtype=np.float64))
            self.off[l["id"]] = (len(theta), v.size, len(theta) + v.size, s.size)
            theta += v.tolist() + s.tolist()
        self.theta = np.array(theta, dtype=np.float64)
        self.inst = [l for g in spec for l in g]
        self.terms = (_native.ExprTerm * len(self.inst))()
        for i, l in enumerate(self.inst):
            vo, nv, lo, nl = self.off[l["id"]]
            self.terms[i] = _native.ExprTerm(_TYPE[l["type"]], _ops.KINDS[l["kind"] or "Rbf"], vo, lo, max(nl, 1), nv)
        starts = np.cumsum([0] + [len(g) for g in spec]).tolist()
        self.gstart = (ctypes.c_int * len(starts))(*starts)
        self.nterms, self.ngroups = len(self.inst), len(spec)

    def head(self):
        return self.terms, self.nterms, self.gstart, self.ngroups

    def nparam(self, i):
        _, nv, _, nl = self.off[self.inst[i]["id"]]
        return nv + nl

    def values(self, i):
        """the constrained values of instance i's parameters, in the sweep's output order"""
        vo, nv, lo, nl = self.off[self.inst[i]["id"]]
        return np.concatenate([self.theta[vo:vo + nv], self.theta[lo:lo + nl]])

    def scaled(self, f):
        """the same structure with every parameter multiplied by f (another model of a lock-step batch)"""
        return _Prog([[dict(l, variance=np.asarray(l["variance"]) * f if np.size(l["variance"]) > 1 else float(l["variance"]) * f,
                            length_scales=None if l["length_scales"] is None else
                            (np.asarray(l["length_scales"]) * f if np.size(l["length_scales"]) > 1 else float(l["length_scales"]) * f))
                       for l in g] for g in self.spec])


def _abi_spec(name, d):
    if name == "lin1*exp+per":          # ONE Linear variance at any d: the sweep's chunked staging of the raw coordinates
        return [[xr.leaf("lin1", "linear", variance=0.5 / math.sqrt(d)), st("exp", "Exp", 1.3, 1.2, d)], [st("per", "Periodic", 0.8, 0.9, d)]]
    return xr.expand_tree(TREES[name][0](d))


ABI_TREES = [("lin+rbf+const", 3), ("(m32+white)*rbf_ard", 16), ("lin1*exp+per", 17), ("lin1*exp+per", 33)]
ABI_N = [1, 64, 65, 130]


def _tile_mask(n, ldk):
    """True where gpn_kernel_matrix_expr writes in lower mode: the 64 x 64 tiles on and below the diagonal, inside the matrix"""
    t = np.arange(n) // 64
    mask = np.zeros((n, ldk), dtype=bool)
    mask[:, :n] = t[:, None] >= t[None, :]
    return mask


def _assemble_lower(p, theta, X, noise, ldk):
    n, d = X.shape
    out = torch.full((n, ldk), float("nan"), dtype=torch.float64, device=X.device)
    st_ = _native.lib().gpn_kernel_matrix_expr(_ops._stream(X.device), *p.head(), _ops._ptr(theta), _ops._ptr(X), n, None, n, d, _ops._ptr(noise),
                                               _ops.GPN_LOWER, _ops._ptr(out), ldk)
    _native.check(st_, "gpn_kernel_matrix_expr")
    return out


@pytest.mark.parametrize("name,d", ABI_TREES)
@pytest.mark.parametrize("n", ABI_N)
def test_abi_lower_assembly_with_noise(device, name, d, n):
    """gpn_kernel_matrix_expr, lower mode, noise on the diagonal, into a NaN-filled buffer with ldk > n: the tiles on and below
    the diagonal hold Kyy, the padding columns and the tiles above the diagonal keep their NaN."""
    spec = _abi_spec(name, d)
    p = _Prog(spec)
    xn = _planted(spec, n + 5 * d, n, d)
    noise, ldk = 0.07, n + 5
    out = _assemble_lower(p, _t(p.theta, device), _t(xn, device), _t([noise], device), ldk).cpu().numpy()
    mask = _tile_mask(n, ldk)
    assert np.all(np.isnan(out[~mask])) and not np.any(np.isnan(out[mask]))
    Kr = xr.expr_K(spec, xn, None) + LD(noise) * np.eye(n, dtype=LD)
    K64 = xr.direct_expr_K(spec, _t(xn), None) + noise * torch.eye(n, dtype=torch.float64)
    m2 = mask[:, :n]
    scale = max(LD(1), np.max(np.abs(Kr)))
    err = float(np.max(np.abs(xr.ld(out[:, :n]) - Kr)[m2]) / scale)
    _hold("b", "K_lower", err, xr.rel_err(K64, Kr), "K")
    assert np.all(np.diag(out[:, :n]) > np.diag(xr.expr_K(spec, xn, None)).astype(np.float64))      # the noise is on the diagonal


def _lml_inputs(n, dy, seed, device, ldg, ldat):
    """a random SPD stand-in for Kyy^-1 (lower triangle only, NaN above and in the padding) and a^T [dy, ldat] (NaN padding)"""
    g = rng.normal(seed, (n, n + 3))
    Q = g @ g.T / (n + 3) + 0.5 * np.eye(n)
    an = rng.normal(seed + 1, (dy, n))
    Kinv = torch.full((_ops.round_up(n, 64), ldg), float("nan"), dtype=torch.float64, device=device)
    Kinv[:n, :n] = _t(np.tril(Q) + np.triu(np.full((n, n), np.nan), 1), device)
    at = torch.full((dy, ldat), float("nan"), dtype=torch.float64, device=device)
    at[:, :n] = _t(an, device)
    return Q, an, Kinv, at


def _sweep(p, theta, i, X, Kinv, at, dy, want_trace):
    n, d = X.shape
    lib = _native.lib()
    work = torch.empty(max(1, int(lib.gpn_kernel_expr_grad_work_bytes(n, n, d, 1)) // 8), dtype=torch.float64, device=X.device)
    out = torch.full((p.nparam(i) + want_trace,), float("nan"), dtype=torch.float64, device=X.device)
    st_ = lib.gpn_kernel_expr_grad(_ops._stream(X.device), *p.head(), _ops._ptr(theta), i, _ops._ptr(X), n, None, n, d, _ops._ptr(Kinv),
                                   Kinv.stride(0), _ops._ptr(at), at.stride(0), dy, want_trace, _ops._ptr(work), _ops._ptr(out))
    _native.check(st_, "gpn_kernel_expr_grad")
    return out


@pytest.mark.parametrize("name,d", ABI_TREES)
@pytest.mark.parametrize("n,dy", [(1, 2), (64, 5), (65, 1), (130, 5), (130, 2)])
def test_abi_lml_mode_sweeps(device, name, d, n, dy):
    """gpn_kernel_expr_grad in LML mode: the weights 1/2 (a a^T - dy Kyy^-1) formed on the fly from the LOWER triangle of a random
    SPD stand-in (NaN everywhere else: nothing else may be read) and a^T [dy, ld], doubled off the diagonal; every leaf instance's
    sweep against the long-double  sum 1/2 (a a^T - dy Kinv) o dK/d theta, and trace(G) from the first instance."""
    spec = _abi_spec(name, d)
    p = _Prog(spec)
    xn = _planted(spec, n + 3 * d, n, d)
    Q, an, Kinv, at = _lml_inputs(n, dy, 700 + n + dy, device, n + 3, n + 5)
    X, theta = _t(xn, device), _t(p.theta, device)
    G = LD(0.5) * (xr.ld(an).T @ xr.ld(an) - dy * xr.ld(Q))
    split = xr.split_instances(spec)
    gr = xr.expr_param_grads(split, xn, None, G)
    G64 = 0.5 * (_t(an).t() @ _t(an) - dy * _t(Q))
    g64 = _direct64(split, xn, None, G64.numpy())[1]
    pos = 0
    for i, l in enumerate([l for g in split for l in g]):
        out = _sweep(p, theta, i, X, Kinv, at, dy, 1 if i == 0 else 0).cpu().numpy()
        assert not np.any(np.isnan(out))
        want = np.concatenate(gr[l["id"]])
        nv = [np.size(v) for v in gr[l["id"]] if np.size(v)]
        got = out[:p.nparam(i)] * p.values(i)                     # d/d theta -> d/d log theta
        e64 = xr.rel_err(torch.cat([t.reshape(-1) for t in g64[pos:pos + len(nv)]]), want)
        pos += len(nv)
        _hold("b", "lml_sweep", xr.rel_err(got, want), e64, "dense_grad")
        if i == 0:
            _hold("b", "lml_trace", xr.rel_err(out[-1], np.trace(G)), xr.rel_err(torch.trace(G64).item(), np.trace(G)), "dense_grad")


@pytest.mark.parametrize("name,d", ABI_TREES)
@pytest.mark.parametrize("n,dy,shared", [(65, 2, False), (130, 5, True), (130, 1, False)])
def test_abi_batched_forms_equal_the_single_calls(device, name, d, n, dy, shared):
    """gpn_kernel_matrix_expr_batched / gpn_kernel_expr_grad_batched for B = 3 models of one structure, each with its own theta,
    own points (sX = n d) or shared ones (sX = 0): per model bit-identical to the single calls -- the assembled lower tiles and
    every sweep's outputs."""
    B = 3
    lib = _native.lib()
    spec = _abi_spec(name, d)
    progs = [_Prog(spec).scaled(f) for f in (1.0, 0.8, 1.3)]
    p = progs[0]
    theta_all = _t(np.stack([q.theta for q in progs]), device)
    xs = [_planted(spec, n + 3 * d + 50 * (0 if shared else b), n, d) for b in range(B)]
    X_all = _t(xs[0] if shared else np.stack(xs), device)
    Xb = lambda b: X_all if shared else X_all[b]
    sX = 0 if shared else n * d
    noise = _t([0.07, 0.02, 0.3], device)
    ldk, rows = n + 5, n + 2
    Kb = torch.full((B, rows, ldk), float("nan"), dtype=torch.float64, device=device)
    st_ = lib.gpn_kernel_matrix_expr_batched(_ops._stream(X_all.device), *p.head(), B, _ops._ptr(theta_all), theta_all.shape[1], _ops._ptr(X_all), sX, n, d,
                                             _ops._ptr(noise), _ops._ptr(Kb), ldk, rows * ldk)
    _native.check(st_, "gpn_kernel_matrix_expr_batched")
    bits = lambda t: t.contiguous().view(torch.int64)
    for b in range(B):
        one = _assemble_lower(p, theta_all[b], Xb(b).contiguous(), noise[b:b + 1], ldk)
        assert torch.equal(bits(Kb[b, :n]), bits(one))                 # NaN where nothing is written, in both
        assert torch.isnan(Kb[b, n:]).all()
    ldg, ldat = n + 3, n + 5
    ins = [_lml_inputs(n, dy, 800 + n + dy + 10 * b, device, ldg, ldat) for b in range(B)]
    Kinv_all = torch.stack([q[2] for q in ins])
    at_all = torch.stack([q[3] for q in ins])
    wb = max(1, int(lib.gpn_kernel_expr_grad_work_bytes(n, n, d, 1)) // 8)
    work = torch.empty(B * wb, dtype=torch.float64, device=device)
    for i in range(p.nterms):
        want_trace = 1 if i == 0 else 0
        nout = p.nparam(i) + want_trace
        o = torch.full((B, nout), float("nan"), dtype=torch.float64, device=device)
        st_ = lib.gpn_kernel_expr_grad_batched(_ops._stream(X_all.device), *p.head(), B, _ops._ptr(theta_all), theta_all.shape[1], i, _ops._ptr(X_all), sX, n, d,
                                               _ops._ptr(Kinv_all), ldg, Kinv_all.stride(0), _ops._ptr(at_all), ldat, at_all.stride(0), dy, want_trace,
                                               _ops._ptr(work), _ops._ptr(o))
        _native.check(st_, "gpn_kernel_expr_grad_batched")
        for b in range(B):
            one = _sweep(p, theta_all[b], i, Xb(b).contiguous(), Kinv_all[b], at_all[b], dy, want_trace)
            assert not torch.isnan(one).any() and torch.equal(o[b], one), (i, b)


# ---- (c) the residual pass --------------------------------------------------------------------------------------------------
def _resid(p, theta, X, noise, a, q0, q1):
    """gpn_refine_resid_part_expr as dist.TileOps.resid_part calls it -> hi + lo of ka [dy, n] in long double"""
    lib = _native.lib()
    n, d = X.shape
    dy, lds = a.shape
    ka = torch.empty(dy, lds, 2, dtype=torch.float64, device=X.device)
    work = torch.empty(max(1, int(lib.gpn_refine_resid_part_work_bytes(dy, q1 - q0)) // 8), dtype=torch.float64, device=X.device)
    st_ = lib.gpn_refine_resid_part_expr(_ops._stream(X.device), *p.head(), _ops._ptr(theta), _ops._ptr(X), n, d, _ops._ptr(noise), _ops._ptr(a), dy,
                                         q0, q1, _ops._ptr(work), _ops._ptr(ka))
    _native.check(st_, "gpn_refine_resid_part_expr")
    ka = xr.ld(ka[:, :n])
    return ka[..., 0] + ka[..., 1]


RESID_TREES = {"lin+rbf+const": (lambda d: xr.expand_tree(TREES["lin+rbf+const"][0](d)), 3),
               "m52*rbf_ard+white": (lambda d: xr.expand_tree(("+", ("*", st("m52", "Matern52", 0.9, 1.1, d), st("rbf", "Rbf", 1.1, 0.8, d, True)),
                                                               white("wh", 0.3))), 5)}


@pytest.mark.parametrize("name", list(RESID_TREES))
@pytest.mark.parametrize("n", [65, 130, 257])
@pytest.mark.parametrize("dy", [1, 3])
def test_residual_pass(device, name, n, dy):
    """gpn_refine_resid_part_expr: Kyy a over the lower tiles and their mirrors, Kyy re-computed from the points, in double-double.
    The whole tile range, and split into two calls whose outputs add up; hi + lo against (1) the long-double Kyy a and (2) the
    product of the matrix gpn_kernel_matrix_expr assembled with a, within the summation error of that long-double product
    n 2^-63 (|Kyy| |a|)_i: the pass reproduces the assembled entries exactly."""
    make, d = RESID_TREES[name]
    spec = make(d)
    p = _Prog(spec)
    xn = _planted(spec, n + 3 * d, n, d)
    noise = 0.07
    an = rng.normal(900 + n + dy, (dy, n))
    lds = _ops.round_up(n, _ops.LEAF)
    a = torch.zeros(dy, lds, dtype=torch.float64, device=device)
    a[:, :n] = _t(an, device)
    X, theta, nz = _t(xn, device), _t(p.theta, device), _t([noise], device)
    ntile = (n + 63) // 64
    ntri = ntile * (ntile + 1) // 2
    assert ntri == int(_native.lib().gpn_refine_tile_count(n))
    whole = _resid(p, theta, X, nz, a, 0, ntri)
    cut = ntri // 2 + 1
    parts = _resid(p, theta, X, nz, a, 0, cut) + _resid(p, theta, X, nz, a, cut, ntri)
    # (1) the long-double Kyy a
    Kyy = xr.expr_K(spec, xn, None) + LD(noise) * np.eye(n, dtype=LD)
    K64 = xr.direct_expr_K(spec, _t(xn), None) + noise * torch.eye(n, dtype=torch.float64)
    want = xr.ld(an) @ Kyy                             # [dy, n]; Kyy symmetric
    e64 = xr.rel_err(xr.ld(an) @ xr.ld(K64), want)
    # (2) the assembled matrix: tiles below the diagonal mirrored, the diagonal tiles as they are (the pass multiplies a diagonal tile
    # entry by entry; with a Linear-ARD leaf its two halves round differently)
    asm = xr.ld(_assemble_lower(p, theta, X, nz, n))
    t = np.arange(n) // 64
    M = np.where(t[:, None] >= t[None, :], asm, asm.T)
    assert not np.any(np.isnan(M))
    exact = M @ xr.ld(an).T                            # [n, dy]
    bound = n * LD(2) ** -63 * (np.abs(M) @ np.abs(xr.ld(an)).T)
    for what, got in (("whole", whole), ("split", parts)):
        _hold("c", "Kyy_a_" + what, xr.rel_err(got, want), e64, "K")
        over = np.max(np.abs(got.T - exact) / bound)
        print("xref c assembled_%s |diff|/bound=%.3e" % (what, float(over)))
        assert over <= 1.0, (what, float(over))


# ---- (d) GPR on the fused path ----------------------------------------------------------------------------------------------
def _gpr_tree(name, d):
    if name == "lin_ard+rbf+const":
        return ("+", ("+", lin("lin", d), st("rbf", "Rbf", 1.2, 0.9, d)), const("c", 0.4))
    if name == "(m52+white)*rbf_ard":
        return ("*", ("+", st("m52", "Matern52", 0.9, 1.1, d), white("wh", 0.3)), st("rbf", "Rbf", 1.1, 0.9, d, True))
    if name == "exp*m32+lin":
        return ("+", ("*", st("exp", "Exp", 1.3, 1.2, d), st("m32", "Matern32", 0.6, 0.9, d)), lin("lin", d))
    if name == "per*rbf+const":
        return ("+", ("*", st("per", "Periodic", 0.8, 1.5, d), st("rbf", "Rbf", 1.3, 0.9, d)), const("c", 0.4))
    raise ValueError(name)


# (tree, n, d, dy, noise: a number or "pd" = 1.5 x what lambda_min(K) lacks of 0, + 0.05, repeated and near-repeated rows)
GPR_CASES = [("lin_ard+rbf+const", 65, 3, 1, 0.05, False), ("(m52+white)*rbf_ard", 129, 16, 5, 0.05, False),
             ("exp*m32+lin", 257, 2, 4, 0.05, True), ("per*rbf+const", 127, 1, 1, "pd", False)]


@pytest.mark.parametrize("c", GPR_CASES, ids=[c[0] for c in GPR_CASES])
def test_gpr_over_an_expression(device, c):
    """GPR over a composite kernel (ExprLogLik: fused assembly into the factor buffer, the LML-mode expression sweeps in the backward)
    against xr.GPRRef over the same spec: loss, the gradient of every raw parameter, the noise and a trainable Constant mean,
    predict_f / predict_y with diag True and False at random points, at training points and far away."""
    name, n, d, dy, noise, special = c
    tree = _gpr_tree(name, d)
    spec = xr.expand_tree(tree)
    x, y = rng.make_regression(n, d, dy, seed=n + d)
    ls0 = _ls0(spec)
    if special:
        x[10:20] = x[:10]                                # repeated rows, near-repeated rows (r ~ 1e-9) ...
        x[20:30] = x[:10] + 1e-9 * ls0
        x[30:34] = 0.0                                   # ... and pairs at r = 1e-21 (under the clamp), 1e-19, 1e-12
        x[31:34, 0] = np.array([1e-21, 1e-19, 1e-12]) * ls0
    if noise == "pd":
        lam = np.linalg.eigvalsh(xr.expr_K(spec, x, None).astype(np.float64)).min()
        noise = 1.5 * max(-lam, 0.0) + 0.05
    mean = np.linspace(-0.3, 0.25, dy)
    lsmax = max(float(np.max(l["length_scales"])) for l in xr.spec_leaves(spec) if l["type"] == "stationary")
    xs = np.concatenate([rng.normal(n + 99, (12, d)), x[:4], 60.0 * lsmax * np.ones((2, d))])
    r = xr.GPRRef(x, y, spec, noise=noise, mean=mean)                  # raises unless Kyy is positive definite
    dg = xr.DirectGPR(x, y, kind=spec, noise=noise, mean=mean)
    objs = {}
    mf = mean_functions.Constant(dy, val=torch.tensor(mean, dtype=torch.float64))
    m = GPR(x, y, _package(tree, d, objs), likelihood=likelihoods.Gaussian(variance=noise), mean_function=mf)
    m.cuda()
    assert type(m.log_likelihood().grad_fn).__name__ == "ExprLogLikBackward"
    m.zero_grad()
    loss = m.loss()
    loss.backward()
    l64, g64 = dg.loss_grads_with_mean()
    _hold("d", "loss", xr.rel_err(loss.item(), r.loss()), xr.rel_err(l64.item(), r.loss()), "loss")
    got = _raw_grads(spec, objs) + [m.likelihood.variance.grad, mf.val.grad]
    want = r.loss_grads()
    assert len(got) == len(want) == len(g64)
    for i, (g, g6, w) in enumerate(zip(got, g64, want)):
        _hold("d", "grad%d" % i, xr.rel_err(g.cpu(), w), xr.rel_err(g6, w), "grad")
    for f in ("predict_f", "predict_y"):
        for diag in (True, False):
            mu, v = getattr(m, f)(xs, diag=diag)
            with torch.no_grad():
                mu64, v64 = getattr(dg, f)(xs, diag)
            mur, vr = getattr(r, f)(xs, diag)
            assert np.shape(mu) == np.shape(mur) and np.shape(v) == np.shape(vr)
            _hold("d", "%s_%s_mean" % (f, diag), xr.abs_err(mu, mur), xr.abs_err(mu64, mur), "mean")
            _hold("d", "%s_%s_var" % (f, diag), xr.abs_err(v, vr), xr.abs_err(v64, vr), "var")
