"""The extended-precision reference (tests/_xref.py) checked on the CPU: against the oracle where the oracle is exact
enough (the smooth kinds), against mpmath at 30 digits entry by entry, against central differences of its own LML, and
-- the point of it -- sharp enough to reject the oracle's own Exp values, whose Gram-trick distances carry sqrt(eps) of
noise into the cusp at r = 0."""
import mpmath
import numpy as np
import pytest
import torch

from gptorch_amd import rng
from oracle import gp_oracle as orc
from tests import _xref as xr

LD = np.longdouble


# ---- against the oracle: the smooth kinds ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,d,dy,ard", [("Rbf", 150, 3, 2, False), ("Matern52", 300, 4, 1, True), ("Matern32", 97, 2, 3, True),
                                             ("Matern32", 1, 2, 1, False), ("Periodic", 211, 1, 2, False)])
def test_matches_the_oracle_on_the_smooth_kinds(kind, n, d, dy, ard):
    x, y = rng.make_regression(n, d, dy, seed=n)
    ls = np.linspace(1.1, 2.0, d) if ard else 1.4
    mean = np.linspace(-0.3, 0.2, dy)
    o = orc.GPROracle(x, y, kind=kind, variance=1.3, length_scales=ls, noise=0.05, ARD=ard, mean=mean)
    o.mean_val.requires_grad_(True)
    loss = o.loss()
    loss.backward()
    r = xr.GPRRef(x, y, kind, 1.3, ls, 0.05, ARD=ard, mean=mean)
    assert xr.rel_err(loss.item(), r.loss()) < 1e-12
    for got, want in zip([o.raw_variance.grad, o.raw_length_scales.grad, o.raw_noise.grad, o.mean_val.grad], r.loss_grads()):
        assert xr.rel_err(got, want) < 1e-12
    xs = np.concatenate([rng.normal(n + 1, (9, d)), x[:3]])
    for diag in (True, False):
        with torch.no_grad():
            for f in ("predict_f", "predict_y"):
                om, ov = getattr(o, f)(xs, diag=diag)
                rm, rv = getattr(r, f)(xs, diag=diag)
                assert xr.abs_err(om, rm) < 1e-12 and xr.abs_err(ov, rv) < 1e-12, (f, diag)
    # ... and K / Kdiag themselves
    with torch.no_grad():
        assert xr.abs_err(o.K(o.X), r.Kf) < 1e-13
        assert xr.abs_err(orc.kernel_Kdiag(o.X, o.raw_variance.exp()), xr.Kdiag(x, 1.3)) == 0.0


# ---- against mpmath, entry by entry ---------------------------------------------------------------------------------
R2 = ["0", "1e-41", "1e-39", "1e-16", "1", str(mpmath.mpf(mpmath.pi) ** 2), "1500", "6e5"]


def _mp_k(kind, r2, v):
    """the reference's definitions (kernels.py:182-235) at 30 digits, clamp included."""
    if kind == "Rbf":
        return v * mpmath.exp(-r2 / 2)
    r = mpmath.sqrt(max(r2, mpmath.mpf("1e-40")))
    if kind == "Matern52":
        s5 = mpmath.sqrt(5)
        return v * (1 + s5 * r + mpmath.mpf(5) / 3 * r * r) * mpmath.exp(-s5 * r)
    if kind == "Matern32":
        s3 = mpmath.sqrt(3)
        return v * (1 + s3 * r) * mpmath.exp(-s3 * r)
    if kind in ("Exp", "Matern12"):
        return v * mpmath.exp(-r)
    return v * mpmath.cos(r)


def _mpf(x):
    return mpmath.mpf(np.format_float_scientific(LD(x), precision=25, unique=False))


@pytest.mark.parametrize("kind", xr.KINDS)
def test_kernel_entries_and_derivatives_against_mpmath(kind):
    """K, dK/dlog(variance) and dK/dlog(ell) at r^2 on both sides of the clamp (1e-40), at the cusp, around pi (Periodic) and
    where exp underflows in fp64 (Rbf at r^2 = 1500, the Exp family at 6e5): the long-double values to a few ulps of
    long double (times the conditioning of exp / cos at the argument)."""
    v = LD("1.3")
    with mpmath.workdps(30):
        vm = _mpf(v)
        for s in R2:
            r2 = LD(s)
            r2m = _mpf(r2)
            Kx, B = xr.k_of_r2(kind, np.array([r2]), v)
            want = _mp_k(kind, r2m, vm)
            # dK/dlog(ell): r^2 scales like ell^-2.  Below the clamp K does not move (the derivative is 0, no diff needed);
            # Rbf takes r^2 itself and has no clamp
            if kind != "Rbf" and r2m < mpmath.mpf("1e-40"):
                dwant = mpmath.mpf(0)
            else:
                with mpmath.workdps(100):          # the change at r^2 ~ 1e-40 is 1e-20 of K and more
                    dwant = mpmath.diff(lambda t: _mp_k(kind, r2m * mpmath.exp(-2 * t), vm), 0)
            dvwant = mpmath.diff(lambda t: _mp_k(kind, r2m, vm * mpmath.exp(t)), 0)
            got, dgot, dvgot = _mpf(Kx[0]), _mpf(B[0] * r2), _mpf(Kx[0])
            # a few long-double ulps times the condition number of exp / cos at the argument (~ r, r^2 for Rbf); cos r has
            # zeros: absolute there.  exp(-3e5) (Rbf at 6e5) is below even long double's range: 1e-4883 absolute
            rel = 2e-18 * (8 + 3 * (r2m if kind == "Rbf" else mpmath.sqrt(r2m)))
            scale = abs(want) + mpmath.mpf("1e-4883") if kind != "Periodic" else vm
            assert abs(got - want) <= rel * scale, (s, got, want)
            assert abs(dvgot - dvwant) <= rel * scale, (s, dvgot, dvwant)
            dscale = abs(dwant) + mpmath.mpf("1e-4883") if kind != "Periodic" else vm * max(1, r2m)
            assert abs(dgot - dwant) <= rel * dscale, (s, dgot, dwant)
            if kind == "Rbf" and s == "1500" or kind in ("Exp", "Matern12") and s == "6e5":
                assert Kx[0] > 0 and np.float64(Kx[0]) == 0.0          # underflows in fp64, not here


def test_matern12_is_exp():
    x, x2 = rng.normal(1, (7, 3)), rng.normal(2, (5, 3))
    assert np.array_equal(xr.K("Matern12", x, x2, 1.3, 0.7), xr.K("Exp", x, x2, 1.3, 0.7))


# ---- closed-form gradients against central differences ------------------------------------------------------------
@pytest.mark.parametrize("kind,d,ard", [("Rbf", 3, True), ("Matern52", 2, False), ("Matern32", 3, True), ("Exp", 3, True),
                                        ("Exp", 2, False), ("Periodic", 1, False)])
def test_closed_form_gradients_against_central_differences(kind, d, ard):
    n, dy = 20, 2
    x, y = rng.make_regression(n, d, dy, seed=7)
    nl = d if ard else 1
    th = np.concatenate([[np.log(LD("1.3"))], np.log(np.linspace(LD("0.8"), LD("1.6"), nl)), [np.log(LD("0.05")), LD("0.2"), LD("-0.1")]])

    def model(t):
        return xr.GPRRef(x, y, kind, np.exp(t[0]), np.exp(t[1:1 + nl]), np.exp(t[1 + nl]), ARD=ard, mean=t[2 + nl:])

    g = np.concatenate(model(th).loss_grads())
    h = LD("1e-5")
    for i in range(len(th)):
        tp, tm = th.copy(), th.copy()
        tp[i] += h
        tm[i] -= h
        fd = (model(tp).loss() - model(tm).loss()) / (2 * h)
        assert abs(fd - g[i]) < 1e-9 * max(1, abs(g[i])), (i, fd, g[i])


# ---- the new checks see what the old judge could not ----------------------------------------------------------------
def test_the_oracle_fails_the_exp_tolerance():
    """Exp, n = 300, d = 3, variance 1.3, ell 1.5, noise 0.05 (inputs x 3): the tolerance the GPU tests apply (16 x the fp64
    direct-difference error, floored) is met by the direct-difference oracle and FAILED by the Gram-trick oracle, whose loss
    and gradients are off by ~1e-8.  A native Exp sweep with an error of that size cannot pass the new tests."""
    n, d, dy = 300, 3, 1
    x, y = rng.make_regression(n, d, dy, seed=0)
    x = 3.0 * x
    kw = dict(kind="Exp", variance=1.3, length_scales=1.5, noise=0.05)
    r = xr.GPRRef(x, y, "Exp", 1.3, 1.5, 0.05)
    want_l, want_g = r.loss(), r.loss_grads()
    dgp = xr.DirectGPR(x, y, **kw)
    l64, g64 = dgp.loss_grads_with_mean()
    e64_l = xr.rel_err(l64.item(), want_l)
    e64_g = max(xr.rel_err(a, b) for a, b in zip(g64, want_g))
    tol_l, tol_g = xr.tol(e64_l, "loss"), xr.tol(e64_g, "grad")
    o = orc.GPROracle(x, y, **kw)
    ol, og = o.loss_and_grads()
    o.mean_val.requires_grad_(True)
    o.loss().backward()
    og = og + [o.mean_val.grad]
    e_l = xr.rel_err(ol.item(), want_l)
    e_g = max(xr.rel_err(a, b) for a, b in zip(og, want_g))
    assert e64_l < tol_l and e64_g < tol_g
    assert e_l > 3 * tol_l, (e_l, tol_l)
    assert e_g > 3 * tol_g, (e_g, tol_g)
    # ... and the K diagonal: the oracle's is off by ~1e-7, the tolerance of the K checks is 1e-13
    with torch.no_grad():
        assert np.max(np.abs(np.diag(o.K(o.X).numpy()) - 1.3)) > 1e3 * xr.FLOOR["K"]
    assert np.all(np.diag(r.Kf) == LD(1.3))                      # v exp(-1e-20): v to long-double precision


# ---- expressions: Sum / Product trees over stationary leaves, Linear, Constant and White ----------------------------
def _expr_spec(d):
    """rbf * m52_ard + lin_ard + white + const, and the rbf leaf once more in  rbf * white * exp_ard  (a leaf in two groups,
    White inside a product)."""
    rbf = xr.leaf("rbf", "stationary", "Rbf", 1.3, 1.4)
    m52 = xr.leaf("m52", "stationary", "Matern52", 0.9, np.linspace(0.8, 1.7, d), ard=True)
    lin = xr.leaf("lin", "linear", variance=np.linspace(0.3, 0.9, d), ard=True)
    wh = xr.leaf("wh", "white", variance=0.25)
    cst = xr.leaf("c", "constant", variance=0.4)
    ex = xr.leaf("exp", "stationary", "Exp", 0.7, np.linspace(1.1, 2.0, d), ard=True)
    return [[rbf, m52], [lin], [wh], [cst], [rbf, wh, ex]]


def _mp_expr(spec, x, x2, sym):
    """the expression for one pair of points at the working precision of mpmath (inputs: float64, exact)."""
    total = mpmath.mpf(0)
    for g in spec:
        prod = mpmath.mpf(1)
        for l in g:
            v = [_mpf(t) for t in np.atleast_1d(l["variance"])]
            if l["type"] == "stationary":
                ls = [_mpf(t) for t in np.atleast_1d(l["length_scales"])]
                r2 = sum(((mpmath.mpf(float(a)) - mpmath.mpf(float(b))) / ls[c % len(ls)]) ** 2 for c, (a, b) in enumerate(zip(x, x2)))
                prod *= _mp_k(l["kind"], r2, v[0])
            elif l["type"] == "linear":
                prod *= sum(mpmath.mpf(float(a)) * v[c % len(v)] * mpmath.mpf(float(b)) for c, (a, b) in enumerate(zip(x, x2)))
            elif l["type"] == "constant":
                prod *= v[0]
            else:
                prod *= v[0] if sym else 0
        total += prod
    return total


def test_expression_value_against_mpmath():
    """expr_K of a tree with a product of two stationary leaves, Linear-ARD, White (alone and inside a product) and Constant,
    entry by entry at 30 digits: K(X) (White on the diagonal only, also where rows repeat) and K(X, X2)."""
    n, m, d = 6, 5, 3
    x, x2 = rng.normal(11, (n, d)), rng.normal(12, (m, d))
    x[4] = x[1]                                         # a repeated row: off the diagonal, no White
    x2[2] = x[0]
    spec = _expr_spec(d)
    Ks, Kx = xr.expr_K(spec, x, None), xr.expr_K(spec, x, x2)
    with mpmath.workdps(30):
        for i in range(n):
            for j in range(n):
                want = _mp_expr(spec, x[i], x[j], i == j)
                assert abs(_mpf(Ks[i, j]) - want) <= 2e-17 * max(1, abs(want)), (i, j)
            for j in range(m):
                want = _mp_expr(spec, x[i], x2[j], False)
                assert abs(_mpf(Kx[i, j]) - want) <= 2e-17 * max(1, abs(want)), (i, j)
    assert Ks[1, 4] == Ks[4, 1] and Ks[1, 1] - Ks[1, 4] > 0.25          # White: the diagonal only
    assert xr.abs_err(xr.expr_Kdiag(spec, x), np.diag(Ks)) < 1e-17          # Linear's sum(x x v) rounds unlike (x v) x^T


def test_white_is_zero_across_two_sets_even_of_the_same_points():
    x = rng.normal(13, (7, 2))
    wh = xr.leaf("wh", "white", variance=0.25)
    assert np.count_nonzero(xr.leaf_K(wh, x, x.copy())) == 0
    assert np.array_equal(xr.leaf_K(wh, x, None), LD(0.25) * np.eye(7, dtype=LD))
    spec = [[wh, xr.leaf("rbf", "stationary", "Rbf", 1.3, 1.4)]]
    assert np.count_nonzero(xr.expr_K(spec, x, x.copy())) == 0
    g = xr.expr_param_grads(spec, x, x.copy(), rng.normal(14, (7, 7)))
    assert all(np.count_nonzero(v) == 0 for pair in g.values() for v in pair)


@pytest.mark.parametrize("sym", [True, False])
def test_expression_gradients_against_central_differences(sym):
    """expr_param_grads (closed form, d/d log theta) against central differences of sum(W * expr_K) in long double: a leaf in
    two groups, White inside a product, Linear-ARD, and the same spec with one shared Linear variance."""
    n, m, d = 9, 7, 3
    x, x2 = rng.normal(21, (n, d)), (None if sym else rng.normal(22, (m, d)))
    W = rng.normal(23, (n, n if sym else m))
    for spec in (_expr_spec(d), [[xr.leaf("lin1", "linear", variance=0.6), xr.leaf("per", "stationary", "Periodic", 0.8, 2.5)]]):
        leaves = xr.spec_leaves(spec)
        g = xr.expr_param_grads(spec, x, x2, W)

        def value(lid, field, c, step):
            mod = [[dict(l, **{field: np.atleast_1d(xr.ld(l[field])) * np.exp(step * (np.arange(np.size(l[field])) == c))})
                    if l["id"] == lid else l for l in grp] for grp in spec]
            return np.sum(xr.ld(W) * xr.expr_K(mod, x, x2))

        h = LD("1e-5")
        checked = 0
        for l in leaves:
            for field, got in zip(("variance", "length_scales"), g[l["id"]]):
                assert np.size(got) == (0 if l[field] is None else np.size(l[field]))
                for c in range(np.size(got)):
                    fd = (value(l["id"], field, c, h) - value(l["id"], field, c, -h)) / (2 * h)
                    assert abs(fd - got[c]) < 1e-9 * max(1, abs(got[c])), (l["id"], field, c, fd, got[c])
                    checked += 1
        assert checked == sum(np.size(l["variance"]) + (0 if l["length_scales"] is None else np.size(l["length_scales"])) for l in leaves)


def test_gpr_reference_accepts_an_expression():
    """GPRRef / DirectGPR over a spec: the closed-form gradients against central differences of the reference's own loss, and
    the fp64 direct evaluation (autograd through direct_expr_K) agreeing with it in loss, gradients and predictions; a
    one-leaf spec reproduces the (kind, variance, length_scales) constructor."""
    n, d, dy = 24, 3, 2
    x, y = rng.make_regression(n, d, dy, seed=5)
    spec = [[xr.leaf("lin", "linear", variance=np.linspace(0.3, 0.9, d), ard=True)], [xr.leaf("rbf", "stationary", "Rbf", 1.2, 1.5)],
            [xr.leaf("c", "constant", variance=0.4)]]
    mean = np.array([0.2, -0.1])
    r = xr.GPRRef(x, y, spec, noise=0.05, mean=mean)
    g = r.loss_grads()
    assert [np.size(v) for v in g] == [d, 1, 1, 1, 1, dy]
    h = LD("1e-5")
    for lid, field, c, got in [("lin", "variance", 1, g[0][1]), ("rbf", "variance", 0, g[1][0]), ("rbf", "length_scales", 0, g[2][0]),
                               ("c", "variance", 0, g[3][0])]:
        def loss(step):
            mod = [[dict(l, **{field: np.atleast_1d(xr.ld(l[field])) * np.exp(step * (np.arange(np.size(l[field])) == c))})
                    if l["id"] == lid else l for l in grp] for grp in spec]
            return xr.GPRRef(x, y, mod, noise=0.05, mean=mean).loss()
        fd = (loss(h) - loss(-h)) / (2 * h)
        assert abs(fd - got) < 1e-9 * max(1, abs(got)), (lid, field, fd, got)
    dg = xr.DirectGPR(x, y, kind=spec, noise=0.05, mean=mean)
    l64, g64 = dg.loss_grads_with_mean()
    assert l64.dtype == torch.float64 and all(t.dtype == torch.float64 for t in g64)
    assert xr.rel_err(l64.item(), r.loss()) < 1e-12
    assert len(g64) == len(g) and all(xr.rel_err(a, b) < 1e-10 for a, b in zip(g64, g))
    xs = np.concatenate([rng.normal(6, (5, d)), x[:2]])
    for f in ("predict_f", "predict_y"):
        for diag in (True, False):
            with torch.no_grad():
                om, ov = getattr(dg, f)(xs, diag=diag)
            rm, rv = getattr(r, f)(xs, diag=diag)
            assert xr.abs_err(om, rm) < 1e-11 and xr.abs_err(ov, rv) < 1e-11, (f, diag)
    one = xr.GPRRef(x, y, [[xr.leaf("k", "stationary", "Matern32", 1.3, 1.4)]], noise=0.05)
    old = xr.GPRRef(x, y, "Matern32", 1.3, 1.4, 0.05)
    assert one.loss() == old.loss() and all(np.array_equal(a, b) for a, b in zip(one.loss_grads(), old.loss_grads()))
