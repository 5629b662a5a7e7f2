"""Leave-one-out GPR in lock step, the part that needs no GPU: the argument validation of the three gpn_loo_*_batched entry points (no
launch), their work-size functions against the single ones, the memory one model of a group is charged, the size rule, and the
group key's new last field -- and the table of lock-step families with every family's key."""
import ctypes

import numpy as np

from gptorch_amd import _native, _ops, kernels, likelihoods, rng
from gptorch_amd.models import EPGP, GPR, VFE, LaplaceGP, _laplace_lockstep, _lockstep, _loo_lockstep


def _host_pointer():
    one = ctypes.c_double(0.0)
    return one, ctypes.cast(ctypes.pointer(one), ctypes.c_void_p)


def test_abi_symbols_exist():
    lib = _native.lib()
    for name in ("gpn_loo_terms_batched", "gpn_loo_terms_batched_work_bytes", "gpn_loo_scale_batched", "gpn_loo_grad_batched",
                 "gpn_loo_grad_batched_work_bytes"):
        assert name in _native.SIGNATURES and hasattr(lib, name), name
    assert hasattr(_ops, "BatchedGPRLooLik")


def test_work_sizes_are_batch_times_the_single_ones():
    lib = _native.lib()
    for n in (0, 1, 256, 257, 8192):
        for batch in (1, 2, 7, 70000):
            assert lib.gpn_loo_terms_batched_work_bytes(n, batch) == batch * lib.gpn_loo_terms_work_bytes(n)
            for nls in (1, 3):
                assert lib.gpn_loo_grad_batched_work_bytes(n, nls, batch) == batch * lib.gpn_loo_grad_work_bytes(n, nls)
    assert lib.gpn_loo_terms_batched_work_bytes(257, 0) == 0 and lib.gpn_loo_grad_batched_work_bytes(257, 1, 0) == 0


def test_terms_batched_rejects_bad_arguments_without_launch():
    """-(argument index), the stream being the first; null pointers and a dummy host address throughout (tests/test_abi.py)."""
    lib = _native.lib()
    keep, p = _host_pointer()
    null = None

    # gpn_loo_terms_batched(stream, batch, n, dy, Kinv, ldk, sK, at, ldat, sAt, work, work_bytes, qt, ldqt, sQt, var, rootd, value)
    def terms(batch=2, n=4, dy=1, Kinv=p, ldk=4, sK=16, at=p, ldat=4, sAt=4, work=p, wb=16, qt=null, ldqt=0, sQt=0):
        return lib.gpn_loo_terms_batched(null, batch, n, dy, Kinv, ldk, sK, at, ldat, sAt, work, wb, qt, ldqt, sQt, null, null, null)

    assert terms(batch=0) == -2 and terms(batch=-3) == -2
    assert terms(n=-1) == -3
    assert terms(dy=0) == -4
    assert terms(Kinv=null) == -5
    assert terms(ldk=3) == -6
    assert terms(sK=15) == -7                      # model 1's block would begin inside model 0's [n, n]
    assert terms(at=null) == -8
    assert terms(ldat=3) == -9
    assert terms(sAt=3) == -10
    assert terms(work=null) == -11
    assert terms(wb=8) == -12                      # two models, one slot
    assert terms(n=257, ldk=257, sK=257 * 257, ldat=257, sAt=257, wb=24) == -12      # two workgroups per model: four slots
    assert terms(qt=p, ldqt=3, sQt=4) == -14
    assert terms(qt=p, ldqt=4, sQt=3) == -15


def test_scale_batched_rejects_bad_arguments_without_launch():
    lib = _native.lib()
    keep, p = _host_pointer()
    null = None

    # gpn_loo_scale_batched(stream, batch, n, Kinv, ldk, sK, rootd, S, lds, sS)
    def scale(batch=2, n=4, Kinv=p, ldk=4, sK=16, rootd=p, S=p, lds=5, sS=20):
        return lib.gpn_loo_scale_batched(null, batch, n, Kinv, ldk, sK, rootd, S, lds, sS)

    assert scale(batch=0) == -2
    assert scale(n=-1) == -3
    assert scale(Kinv=null) == -4
    assert scale(ldk=3) == -5
    assert scale(sK=15) == -6
    assert scale(rootd=null) == -7
    assert scale(S=null) == -8
    assert scale(lds=3) == -9
    assert scale(sS=18) == -10                     # (n - 1) lds + n = 19 doubles of model 0 are written
    assert scale(n=0, ldk=0, sK=0, lds=0, sS=0) == 0            # nothing to do, nothing launched


def test_grad_batched_rejects_bad_arguments_without_launch():
    lib = _native.lib()
    keep, p = _host_pointer()
    null = None
    ok = lib.gpn_loo_grad_batched_work_bytes(4, 1, 2)
    assert ok == 2 * 3 * 8

    # gpn_loo_grad_batched(stream, kind, batch, X, sX, n, d, variance, length_scales, nls, Q, ldq, sQ, at, ldat, sAt, wt, ldwt, sWt, dy,
    #                      work, work_bytes, out)
    def grad(kind=0, batch=2, X=p, sX=0, n=4, d=2, var=p, ls=p, nls=1, Q=p, ldq=4, sQ=16, at=p, ldat=4, sAt=4, wt=p, ldwt=4, sWt=4, dy=1,
             work=p, wb=ok, out=p):
        return lib.gpn_loo_grad_batched(null, kind, batch, X, sX, n, d, var, ls, nls, Q, ldq, sQ, at, ldat, sAt, wt, ldwt, sWt, dy, work, wb, out)

    assert grad(kind=6) == -2 and grad(kind=-1) == -2          # a bad kind
    assert grad(batch=0) == -3
    assert grad(X=null) == -4
    assert grad(sX=7) == -5                        # neither shared (0) nor a whole [n, d] block
    assert grad(n=-1) == -6
    assert grad(d=0) == -7
    assert grad(var=null) == -8
    assert grad(ls=null) == -9
    assert grad(nls=3) == -10 and grad(d=3, nls=2) == -10      # nls not in {1, d}
    assert grad(Q=null) == -11
    assert grad(ldq=3) == -12
    assert grad(sQ=15) == -13
    assert grad(at=null) == -14
    assert grad(ldat=3) == -15
    assert grad(sAt=3) == -16
    assert grad(wt=null) == -17
    assert grad(ldwt=3) == -18
    assert grad(sWt=3) == -19
    assert grad(dy=0) == -20
    assert grad(work=null) == -21
    assert grad(wb=ok - 8) == -22
    assert grad(out=null) == -23


def test_per_model_bytes_is_the_sum_of_the_librarys_sizes():
    lib = _native.lib()
    for n, dy, nls in ((1, 1, 1), (300, 1, 1), (257, 2, 3), (513, 5, 2), (8192, 1, 8)):
        ld, ld0 = lib.gpn_factor_ld(n, dy), lib.gpn_factor_ld(n, 0)
        want = 8 * lib.gpn_factor_rows(n, dy) * ld + max(16, lib.gpn_winv_bytes(n))              # the model's slot of the FactorBatch
        want += lib.gpn_lml_kinv_batched_work_bytes(n, dy, 1)                                     # U (later S), P, a^T
        want += 8 * _ops.round_up(n, 64) * ld0                                                   # Q
        want += 8 * _ops.round_up(dy, 128) * ld                                                  # the right-hand sides of w
        want += lib.gpn_loo_grad_batched_work_bytes(n, nls, 1) + lib.gpn_loo_terms_batched_work_bytes(n, 1)
        want += 8 * (dy * n + 2 * n)                                                             # w^T, 1 / p, sqrt d
        assert _loo_lockstep.per_model_bytes(n, dy, nls) == want
        # four padded N x N matrices and change: never a fifth
        assert want < 5 * 8 * lib.gpn_factor_rows(n, dy) * ld + (1 << 20)


def test_size_rule():
    assert not _loo_lockstep.supported(0) and not _loo_lockstep.supported(_loo_lockstep.MAX_N + 1)
    assert _loo_lockstep.supported(1) and _loo_lockstep.supported(_loo_lockstep.MAX_N)


def test_group_key_keeps_its_positions():
    key = _lockstep.GroupKey("Rbf", (300, 2), 1, 1, "cpu")
    assert key.objective == "lml" and key[5] is None and key._fields[5] == "sizes" and key._fields[-1] == "objective"
    ragged = _lockstep.GroupKey("Rbf", (300, 2), 1, 1, "cpu", (300, 299))
    assert ragged[5] == (300, 299) and ragged.objective == "lml"
    assert key._replace(objective="loo") != key


def test_plan_of_cpu_models_is_an_empty_list():
    x, y = rng.make_regression(20, 2, 1, seed=5)
    ms = [GPR(x, y, kernels.Rbf(2), objective="loo"), GPR(x, y, kernels.Rbf(2), objective="loo"), GPR(x, y, kernels.Rbf(2))]
    assert _lockstep._plan_groups(ms) == []
    assert _lockstep._loo_groups(ms) == []


def test_family_table_on_cpu_models():
    """one CPU-resident model of each family: no family takes any of them, the table is the six families in the order in which
    the entry points evaluate them, and every family's key is a hashable named tuple whose fields have names"""
    x, y = rng.make_regression(20, 2, 1, seed=5)
    labels = (np.asarray(y) > 0).astype(np.float64)
    composite = GPR(x, y, kernels.Rbf(2) + kernels.Matern52(2))
    vfe = VFE(x, y, kernels.Rbf(2), inducing_points=x[:8])
    laplace = LaplaceGP(x, labels, kernels.Rbf(2), likelihoods.Bernoulli("probit"))
    ep = EPGP(x, labels, kernels.Rbf(2), likelihoods.Bernoulli("logit"))
    ms = [GPR(x, y, kernels.Rbf(2)), GPR(x, y, kernels.Rbf(2), objective="loo"), composite, vfe, laplace, ep]
    assert _lockstep._plan_groups(ms) == []
    assert [family.name for family in _lockstep.FAMILIES] == ["lml", "loo", "expr", "vfe", "laplace", "ep"]
    for family in _lockstep.FAMILIES:
        assert family.groups(ms) == [] and family.groups(ms, for_grad=True) == [], family.name
    prog = composite.kernel.fused_program()                                   # (GPR._expression hands it out on the GPU only)
    keys = {"lml": _lockstep._group_key(ms[0]),
            "loo": _lockstep._group_key(ms[1])._replace(objective="loo"),
            "expr": _lockstep.ExprKey("expr", prog.signature(), tuple(composite.X.shape), 1, composite.X.device),
            "vfe": _lockstep.VFEKey("vfe", "Rbf", tuple(vfe.X.shape), 1, 1, tuple(vfe.Z.shape), vfe.X.device),
            "laplace": _lockstep._laplace_key(laplace),
            "ep": _lockstep._ep_key(ep)}
    fields = {"lml": ("kind", "shape", "dy", "nls", "device", "sizes", "objective"),
              "expr": ("tag", "signature", "shape", "dy", "device"),
              "vfe": ("tag", "kind", "shape", "dy", "nls", "z_shape", "device"),
              "laplace": ("tag", "kind", "lik_kind", "shape", "nls", "device", "H")}
    fields["loo"], fields["ep"] = fields["lml"], fields["laplace"]
    assert sorted(keys) == sorted(family.name for family in _lockstep.FAMILIES)
    for name, key in keys.items():
        assert isinstance(key, tuple) and key._fields == fields[name], name
        assert all(getattr(key, field) == value for field, value in zip(key._fields, key)), name
        assert hash(key) == hash(tuple(key)) and {key: 1}[key] == 1, name
    assert len({tuple(key) for key in keys.values()}) == 6          # (no two families' keys compare equal)
    assert keys["expr"].tag == "expr" and keys["vfe"].tag == "vfe" and keys["laplace"].tag == "laplace" and keys["ep"].tag == "ep"
    assert keys["loo"].objective == "loo" and keys["vfe"].z_shape == (8, 2) and keys["ep"].H == ep.likelihood.num_gauss_hermite_points
    assert keys["laplace"].H is None and type(keys["laplace"]) is type(keys["ep"]) is _lockstep.SiteKey
    # the one byte count of three padded N x N matrices serves the stationary capacity rule and LaplaceGP's
    assert _lockstep.three_padded_matrices_bytes(300) == 3 * 8 * (512 + 16) * 512 == _laplace_lockstep.per_model_bytes(300)
