"""The k-fold objective of GPR, the part that needs no GPU: the host oracle's closed form against real refits, against the
leave-one-out oracle (all-singleton folds) and against central differences of its own long-double value; the `folds` and
`objective` keywords; the lock-step grouping helpers; the argument validation of every gpn_kfold_* entry point (no launch)."""
import json

import numpy as np
import pytest

from gptorch_amd import _native, _ops, kernels, rng
from gptorch_amd.models import GPR
from tests import _kfold_oracle as ko
from tests import _loo_oracle as lo
from tests import _xref as xr
from tests._util import load_npz
from tests.golden import make_kfold_golden as maker

GOLD = load_npz("kfold_cases.npz")
CASES = {c["name"]: c for c in json.loads(str(GOLD["meta"]))["cases"]}
EPS = 2.0 ** -52
LD = ko.LD


def test_golden_folds_are_the_makers():
    for name, case in CASES.items():
        parts = ko.partition(maker.case_folds(case), case["n"])
        assert np.array_equal(np.concatenate(parts), GOLD[name + "__folds_idx"])
        assert np.array_equal(np.concatenate([[0], np.cumsum([p.size for p in parts])]), GOLD[name + "__folds_off"])


@pytest.mark.parametrize("name", ["rbf_ard_203x8_shuffled_dy5", "exp_64x17_63_1_dy5"])
def test_closed_form_equals_refits(name):
    """Both sides in long double: every fold's log density, and its held-out means and variances, in closed form against a model
    refitted WITHOUT the fold (a fresh factorisation of the other rows, the full predictive covariance, the multivariate normal
    density) -- the value to 1e-15 relative, means and variances to 1e-14 (the maker's bounds); the stored refits (rounded to fp64:
    2^-53 by itself) to 2^-52."""
    case = CASES[name]
    ref, _ = maker.build(case)
    mean, var = ref.kfold_predict()
    total = LD(0)
    k = len(ref.parts)
    for f, I in enumerate(ref.parts):
        logp, m, v = ref.refit(f)
        total += logp
        assert abs(logp - ref.fold_log_density(f)) <= 1e-15 * max(1, abs(logp))
        assert xr.rel_err(m, mean[I]) <= 1e-14 and xr.rel_err(v, var[I, 0]) <= 1e-14
        if f in (0, k - 1):
            tag = "first" if f == 0 else "last"
            assert xr.rel_err(mean[I], GOLD["%s__refit_%s_mean" % (name, tag)]) <= EPS
            assert xr.rel_err(var[I, 0], GOLD["%s__refit_%s_var" % (name, tag)]) <= EPS
    err = float(abs(total - ref.kfold()) / max(1, abs(ref.kfold())))
    print("%s: sum of refit log densities vs closed form %.2e" % (name, err))
    assert err <= 1e-15


def test_singleton_folds_are_leave_one_out():
    """every m_f = 1: value, predictions and gradients of tests/_loo_oracle.LooRef to 1e-15 relative, both in long double"""
    n, d, dy = 40, 3, 2
    x, y = rng.make_regression(n, d, dy, seed=41)
    args = (x, y, "Matern52", 1.3, [0.9, 1.4, 0.7], 0.04)
    kf = ko.KFoldRef(*args, ARD=True, mean=[0.25, -0.1], folds=[[i] for i in range(n)])
    loo = lo.LooRef(*args, ARD=True, mean=[0.25, -0.1])
    assert abs(kf.kfold() - loo.loo()) <= 1e-15 * max(1, abs(loo.loo()))
    for got, want in zip(kf.kfold_predict(), loo.loo_predict()):
        assert xr.rel_err(got, want) <= 1e-15
    for got, want in zip(kf.loss_grads(), loo.loss_grads()):
        assert xr.rel_err(got, want) <= 1e-15


def test_oracle_gradient_matches_central_differences():
    """d(-L_kfold)/d(log variance, log ell (ARD), log noise, mean) in closed form against central differences of the long-double
    value.  Step h = 1e-4: truncation h^2 / 6 |f'''| = 1.7e-9 |f'''|, rounding 2 eps |loss| / h ~ 1e-13 with eps = 2^-64.  The bound
    1e-6 max(1, |g|) leaves room for |f'''| up to 600 (tests/test_loo_host.py uses the same step and bound)."""
    n, d, dy, h = 40, 3, 2, 1e-4
    x, y = rng.make_regression(n, d, dy, seed=41)
    order = np.argsort(rng.uniform(43, n), kind="stable")
    folds = [order[:17], order[17:30], order[30:]]
    theta0 = np.array([np.log(1.3), np.log(0.9), np.log(1.4), np.log(0.7), np.log(0.04), 0.25, -0.1])

    def oracle(theta):
        t = np.asarray(theta, dtype=LD)
        return ko.KFoldRef(x, y, "Matern52", np.exp(t[0]), np.exp(t[1:4]), np.exp(t[4]), ARD=True, mean=t[5:7], folds=folds)

    got = np.concatenate([np.asarray(g, dtype=np.float64).ravel() for g in oracle(theta0).loss_grads()])
    for i in range(theta0.size):
        e = np.zeros_like(theta0)
        e[i] = h
        fd = float((oracle(theta0 + e).loss() - oracle(theta0 - e).loss()) / (2 * LD(h)))
        print("d/dtheta[%d]: closed %.10f central %.10f" % (i, got[i], fd))
        assert abs(got[i] - fd) <= 1e-6 * max(1.0, abs(fd))


def test_fp64_statement_agrees_with_the_long_double_one():
    """the two host statements of a small model under the suite's floors (tests/_xref.FLOOR) -- what makes e64 a yardstick."""
    x, y = rng.make_regression(60, 2, 2, seed=43)
    ref, t64 = ko.make_pair(x, y, "Exp", 1.1, 0.9, 0.05, mean=[0.1, 0.2], folds=4)
    loss, grads = t64.loss_grads_with_mean()
    assert xr.rel_err(loss, ref.loss()) <= xr.FLOOR["loss"]
    for g, want in zip(grads, ref.loss_grads()):
        assert xr.rel_err(g, want) <= xr.FLOOR["grad"]
    for got, want, what in zip(t64.kfold_predict(), ref.kfold_predict(), ("mean", "var")):
        assert xr.abs_err(got, want) <= xr.FLOOR[what]


# ---- the keywords -----------------------------------------------------------------------------------------------------------------
def test_folds_keyword():
    n = 20
    x, y = rng.make_regression(n, 2, 1, seed=5)
    k = lambda: kernels.Rbf(2)
    m = GPR(x, y, k(), objective="kfold", folds=3)
    assert m.objective == "kfold" and m.folds.k == 3 and m.folds.sizes == (7, 7, 6) and m.folds.m_max == 7
    want = np.array_split(np.arange(n), 3)
    assert all(np.array_equal(p, w) for p, w in zip(m.folds.parts, want))           # the int form IS array_split: contiguous, in data order
    assert m.folds._off.tolist() == [0, 7, 14, 20] and m.folds._idx.tolist() == list(range(n))
    order = np.argsort(rng.uniform(9, n), kind="stable")
    lists = [order[:9], order[9:12], order[12:]]
    m = GPR(x, y, k(), objective="kfold", folds=lists)
    assert m.folds.sizes == (9, 3, 8) and m.folds._idx.tolist() == order.tolist()    # the order given is kept: no sorting
    assert GPR(x, y, k(), objective="kfold", folds=[list(range(10)), range(10, 20)]).folds.k == 2
    bad = {
        "overlap": [np.arange(0, 11), np.arange(10, 20)],
        "gap": [np.arange(0, 9), np.arange(10, 20)],
        "empty fold": [np.arange(0, 20), np.arange(0)],
        "k = 1 (lists)": [np.arange(0, 20)],
        "k = 1 (int)": 1,
        "k > n": 21,
        "out of range": [np.arange(0, 10), np.arange(11, 21)],
        "negative": [np.arange(-1, 10), np.arange(10, 19)],
        "floats": [np.arange(0, 10) * 1.0, np.arange(10, 20) * 1.0],
    }
    for what, folds in bad.items():
        with pytest.raises(ValueError):
            GPR(x, y, k(), objective="kfold", folds=folds)
            pytest.fail(what)
    with pytest.raises(ValueError, match="folds"):
        GPR(x, y, k(), objective="kfold")                                           # missing
    with pytest.raises(ValueError, match="folds"):
        GPR(x, y, k(), objective="loo", folds=3)                                    # folds belongs to "kfold"
    with pytest.raises(ValueError):
        m.kfold_log_predictive(folds=[np.arange(0, 11), np.arange(10, 20)])
    assert GPR(x, y, k()).folds is None and GPR(x, y, k()).objective == "lml"


def test_padding_rule():
    """k * round_up(m_max, 16) > 4 round_up(n, 16): refused, pointing at objective="loo" -- 65 singleton folds (65 * 16 > 320, and
    > 4 * 65 = 260 as well) and a lopsided partition; the edge shapes of the GPU suite, n = 7 with k = 2 among them, are within the rule."""
    x, y = rng.make_regression(65, 2, 1, seed=5)
    with pytest.raises(NotImplementedError, match="loo"):
        GPR(x, y, kernels.Rbf(2), objective="kfold", folds=[[i] for i in range(65)])
    with pytest.raises(NotImplementedError, match="loo"):
        GPR(x, y, kernels.Rbf(2), objective="kfold", folds=65)
    with pytest.raises(NotImplementedError, match="loo"):
        _ops.FoldTable([np.arange(40)] + [[i] for i in range(40, 65)], 65)          # 26 * 48 > 320
    assert _ops.FoldTable([np.arange(63), [63]], 64).m_max == 63                     # 2 * 64 <= 256
    for name, case in CASES.items():
        t = _ops.FoldTable(maker.case_folds(case), case["n"])
        assert t.k * _ops.round_up(t.m_max, 16) <= 4 * _ops.round_up(case["n"], 16), name


def test_objective_keyword():
    x, y = rng.make_regression(20, 2, 1, seed=5)
    for bad in ("bogus", "KFOLD", "k-fold", None):
        with pytest.raises(ValueError, match="objective"):
            GPR(x, y, kernels.Rbf(2), objective=bad, folds=2)
    assert GPR(x, y, kernels.Rbf(2), objective="loo").objective == "loo"
    from gptorch_amd.models.dist_gpr import DistGPR
    with pytest.raises(NotImplementedError):
        DistGPR(x, y, kernels.Rbf(2), objective="kfold")
    with pytest.raises(NotImplementedError, match="leave-one-out"):
        DistGPR(x, y, kernels.Rbf(2), objective="loo")


def test_lockstep_grouping_leaves_kfold_models_alone():
    """the grouping helpers of batched_loss_and_grad / multi_start_optimize / batched_log_likelihood never take a k-fold model
    (decided before anything touches a device: the filters come first)."""
    from gptorch_amd.models import _lockstep
    x, y = rng.make_regression(20, 2, 1, seed=5)
    ms = [GPR(x, y, kernels.Rbf(2)), GPR(x, y, kernels.Rbf(2), objective="kfold", folds=2), GPR(x, y, kernels.Rbf(2)),
          GPR(x, y, kernels.Rbf(2), objective="kfold", folds=2)]
    assert _lockstep._lockstep_groups(ms, for_grad=True) == [] and _lockstep._lockstep_groups(ms) == []   # (CPU-resident models form no group at all)
    assert _lockstep._loo_groups(ms) == []
    masked = [m if m.objective == "lml" else None for m in ms]
    assert _lockstep._lockstep_groups(masked) == [] and _lockstep._expression_groups(masked) == []

    class OnDevice:
        """what the filters look at, without a device: is_cuda, a shape and a device to key on"""
        is_cuda, shape, device = True, (20, 2), "none"

    # pretend the models sit on a GPU: the two ordinary ones pair up, the two k-fold ones never do
    for m in ms:
        m.X = OnDevice()
    for for_grad in (True, False):
        assert [g for _key, g in _lockstep._lockstep_groups(ms, for_grad=for_grad)] == [[0, 2]]
    assert _lockstep._loo_groups(ms) == []
    sums = [GPR(x, y, kernels.Rbf(2) + kernels.Rbf(2), objective="kfold", folds=2) for _ in range(2)]
    for m in sums:
        m.X = OnDevice()
    assert _lockstep._expression_groups(sums) == []


# ---- the entry points' argument validation ------------------------------------------------------------------------------------------
def test_argument_validation_without_launch():
    """every gpn_kfold_* entry point rejects bad arguments with -(argument index) / GPN_E_* before any HIP call (null pointers and
    a dummy host address throughout, as tests/test_loo_host.py does for its neighbours)."""
    import ctypes
    lib = _native.lib()
    null = None
    one = ctypes.c_double(0.0)
    p = ctypes.cast(ctypes.pointer(one), ctypes.c_void_p)
    E_ALIGN, E_UNSUPPORTED = -101, -102
    ld, rows = int(lib.gpn_factor_ld(40, 2)), int(lib.gpn_factor_rows(40, 2))
    assert (ld, rows) == (128, 144)

    def gather(n=100, dy=2, Kinv=p, ldk=100, at=p, ldat=100, k=3, off=p, idx=p, m_max=40, A=p, lda=ld, sA=rows * ld):
        return lib.gpn_kfold_gather(null, n, dy, Kinv, ldk, at, ldat, k, off, idx, m_max, A, lda, sA)

    assert gather(n=0) == -2 and gather(n=1 << 31) == -2
    assert gather(dy=0) == -3
    assert gather(Kinv=null) == -4
    assert gather(ldk=99) == -5
    assert gather(at=null) == -6
    assert gather(ldat=99) == -7
    assert gather(k=0) == -8
    assert gather(k=65536) == E_UNSUPPORTED
    assert gather(off=null) == -9
    assert gather(idx=null) == -10
    assert gather(m_max=0) == -11 and gather(m_max=101) == -11
    assert gather(A=null) == -12
    assert gather(lda=ld - 1) == -13
    assert gather(sA=rows * ld - 1) == -14

    aligned = ctypes.c_void_p(1 << 20)                       # never dereferenced: validation only

    def columns(n=100, Kinv=p, ldk=100, k=3, off=p, idx=p, m_max=40, C=aligned, ldc=48, sC=112 * 48):
        return lib.gpn_kfold_columns(null, n, Kinv, ldk, k, off, idx, m_max, C, ldc, sC)

    assert columns(n=0) == -2
    assert columns(Kinv=null) == -3
    assert columns(ldk=99) == -4
    assert columns(k=0) == -5
    assert columns(k=65536) == E_UNSUPPORTED
    assert columns(off=null) == -6
    assert columns(idx=null) == -7
    assert columns(m_max=0) == -8 and columns(m_max=101) == -8
    assert columns(C=null) == -9
    assert columns(ldc=47) == -10
    assert columns(sC=112 * 48 - 2) == -11
    assert columns(ldc=49, sC=112 * 49) == E_ALIGN
    assert columns(C=ctypes.c_void_p((1 << 20) + 8)) == E_ALIGN
    assert lib.gpn_kfold_columns_work_bytes(100, 3, 40) == 3 * 112 * 48 * 8 and lib.gpn_kfold_columns_work_bytes(0, 3, 40) == 0

    def terms(n=100, dy=2, k=3, off=p, idx=p, m_max=40, U=p, ldu=ld, sU=rows * ld, A=p, lda=ld, sA=rows * ld, out3=p, info=p, qt=null, ldqt=0,
              var=null, Wt=null, ldw=0, sW=0, value=null):
        return lib.gpn_kfold_terms(null, n, dy, k, off, idx, m_max, U, ldu, sU, A, lda, sA, out3, info, qt, ldqt, var, Wt, ldw, sW, value)

    assert terms(n=0) == -2
    assert terms(dy=0) == -3
    assert terms(k=0) == -4
    assert terms(k=65536) == E_UNSUPPORTED
    assert terms(off=null) == -5
    assert terms(idx=null) == -6
    assert terms(m_max=0) == -7 and terms(m_max=101) == -7
    assert terms(U=null) == -8
    assert terms(ldu=39) == -9
    assert terms(sU=40 * ld - 1) == -10
    assert terms(A=null) == -11
    assert terms(lda=ld - 1) == -12
    assert terms(sA=rows * ld - 1) == -13
    assert terms(out3=null, value=p) == -14
    assert terms(qt=p, ldqt=99) == -17
    assert terms(Wt=p, ldw=47, sW=48 * 48) == -20
    assert terms(Wt=p, ldw=48, sW=48 * 48 - 1) == -21
    assert terms() == 0                                      # every output NULL: nothing to do, nothing launched
    assert lib.gpn_kfold_weights_work_bytes(3, 40, 2) == 3 * 48 * 48 * 8 and lib.gpn_kfold_weights_work_bytes(0, 40, 2) == 0
