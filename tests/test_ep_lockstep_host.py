"""EPGP in lock step, the part that needs no GPU: the new entry point is declared, exported and bound, it validates its arguments
before any launch, its workspace is `batch` times the single one, the grouping keeps apart what must not share a call, and the
inputs of the GPU tests' searches have the properties those tests rely on (the CPU oracle's sweep counts and stall)."""
import ctypes
import json
import os
import re

import numpy as np
import torch

from gptorch_amd import _native, _ops, kernels, likelihoods, rng
from gptorch_amd.models import EPGP, LaplaceGP
from gptorch_amd.models import _ep_lockstep as el
from gptorch_amd.models import _lockstep
from tests import _ep_oracle as eo
from tests import _laplace_oracle as lo
from tests._util import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gpn_ep_sites_batched_work_bytes", "gpn_ep_sites_batched"]
UNSUPPORTED = -102
P = ctypes.c_void_p(64)         # a non-null "pointer": every call below returns before anything could follow it
CASES = {c["name"]: c for c in json.loads(str(load_npz("ep_cases.npz")["meta"]))["cases"]}
SETTINGS = ((0.3, 1.0), (1.7, 1.0), (8.0, 0.5))       # (variance, length-scale) of the GPU tests' three restarts


def test_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpnative.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gpn_\w+)\s*\(", text))
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
    assert callable(_ops.ep_sites_batched)
    assert set(el.STATS) == {"searches", "sweeps", "reads", "factorisations"}
    assert callable(el.find_sites_batched) and callable(el.supported) and callable(el.per_model_bytes)
    assert issubclass(el.BatchedEPEvidence, torch.autograd.Function)
    assert callable(_lockstep._ep_groups) and callable(_lockstep._ep_key)


def test_argument_validation_without_launch():
    """-(argument index), the stream being argument 1, before any HIP call; Poisson / Student-t and a batch beyond a grid
    dimension: GPN_E_UNSUPPORTED"""
    lib = _native.lib()
    null = None
    names = ("kind", "batch", "n", "y", "sy", "m", "mu", "sigma2", "tau", "nu", "dampings", "nodes", "weights", "H", "moments_only",
             "work", "work_bytes", "tau_out", "nu_out", "lz", "mu_hat", "s2_hat", "stats")
    good = dict(kind=_native.LIK_PROBIT, batch=2, n=300, y=P, sy=0, m=null, mu=P, sigma2=P, tau=P, nu=P, dampings=P, nodes=null,
                weights=null, H=0, moments_only=0, work=P, work_bytes=2 * 2 * 6 * 8, tau_out=P, nu_out=P, lz=null, mu_hat=null,
                s2_hat=null, stats=null)         # (stats, the LAST argument checked, stays null: nothing is ever launched)

    def call(**over):
        a = dict(good, **over)
        return lib.gpn_ep_sites_batched(null, *[a[k] for k in names])

    assert call() == -24                                                   # everything before the last argument passes
    assert call(kind=7) == -2 and call(kind=-1) == -2
    assert call(kind=_native.LIK_POISSON) == UNSUPPORTED and call(kind=_native.LIK_STUDENT_T) == UNSUPPORTED
    assert call(batch=0) == -3 and call(batch=-2) == -3
    assert call(batch=65536, work_bytes=1 << 40) == UNSUPPORTED and call(batch=65535, work_bytes=1 << 40) == -24
    assert call(n=0) == -4
    # null pointers, in argument order (m may be null: a zero mean)
    for k, code in (("y", -5), ("mu", -8), ("sigma2", -9), ("tau", -10), ("nu", -11), ("dampings", -12), ("work", -17),
                    ("tau_out", -19), ("nu_out", -20)):
        assert call(**{k: null}) == code, k
    assert call(sy=7) == -6 and call(sy=300) == -24                        # targets: shared (0) or stacked (n)
    assert call(moments_only=1, tau_out=null, nu_out=null) == -24           # no update: no site outputs needed
    # logit needs its rule, 2 <= H <= 64
    logit = dict(kind=_native.LIK_LOGIT)
    assert call(**logit) == -13 and call(nodes=P, **logit) == -14
    for H, code in ((0, -15), (1, -15), (65, -15), (2, -24), (20, -24), (64, -24)):
        assert call(nodes=P, weights=P, H=H, **logit) == code, H
    assert call(work_bytes=2 * 2 * 6 * 8 - 1) == -18


def test_workspace_is_batch_times_the_single_one():
    lib = _native.lib()
    for n in (1, 256, 257, 300, 65537):
        for batch in (1, 3, 64):
            assert lib.gpn_ep_sites_batched_work_bytes(n, batch) == batch * lib.gpn_ep_sites_work_bytes(n)
    assert lib.gpn_ep_sites_batched_work_bytes(300, 0) == 0 and lib.gpn_ep_sites_batched_work_bytes(0, 4) == 0


def _ep(n, kernel, lik, seed=1, H=None):
    x = rng.normal(seed, (n, 2))
    y = (rng.uniform(seed + 1, n) < 0.5).astype(np.float64).reshape(n, 1)
    if H is not None:
        lik.num_gauss_hermite_points = H
    return EPGP(x, y, kernel, lik)


def test_grouping_on_the_host():
    base = [_ep(30, kernels.Rbf(2), likelihoods.Bernoulli("probit"), seed=s) for s in (1, 2)]
    assert _lockstep._ep_groups(base) == []                               # CPU-resident models: nothing to run in lock step
    assert _lockstep._laplace_groups(base) == []                          # ... and never a LaplaceGP group
    assert _lockstep._ep_key(base[0]) == _lockstep._ep_key(base[1])
    others = [_ep(30, kernels.Rbf(2), likelihoods.Bernoulli("logit"), H=20),              # link
              _ep(30, kernels.Rbf(2), likelihoods.Bernoulli("logit"), H=32),              # H, for logit
              _ep(30, kernels.Matern52(2), likelihoods.Bernoulli("probit")),              # kernel kind
              _ep(30, kernels.Rbf(2, ARD=True), likelihoods.Bernoulli("probit")),         # ARD
              _ep(31, kernels.Rbf(2), likelihoods.Bernoulli("probit"))]                   # N
    keys = [_lockstep._ep_key(m) for m in [base[0]] + others]
    assert len(set(keys)) == len(keys) and all(k.tag == "ep" for k in keys)
    assert keys[1].H == 20 and keys[2].H == 32 and keys[0].H == 0
    # probit's moments are closed form: models that differ in the likelihood's quadrature setting alone stay together
    assert _lockstep._ep_key(_ep(30, kernels.Rbf(2), likelihoods.Bernoulli("probit"), H=32)) == keys[0]
    # LaplaceGP models never enter an EP group, whatever else the list holds
    x, y = rng.normal(1, (30, 2)), (rng.uniform(2, 30) < 0.5).astype(np.float64).reshape(30, 1)
    lap = [LaplaceGP(x, y, kernels.Rbf(2), likelihoods.Bernoulli("probit")) for _ in range(2)]
    assert _lockstep._ep_groups(lap + base) == []
    assert not any(isinstance(m, EPGP) for m in lap) and not any(isinstance(m, LaplaceGP) for m in base)
    plan = _lockstep._plan_groups(lap + base)
    assert isinstance(plan, list) and not [grp for grp in plan if grp.family.name in ("laplace", "ep")]
    assert el.supported(1) and el.supported(512) and el.supported(el.MAX_N) and not el.supported(0) and not el.supported(el.MAX_N + 1)


def test_per_model_bytes_come_from_the_library():
    lib = _native.lib()
    for n, nls in ((300, 1), (512, 3), (2048, 1)):
        slot = 8 * lib.gpn_factor_rows(n, 1) * lib.gpn_factor_ld(n, 1) + lib.gpn_winv_bytes(n)
        want = slot + lib.gpn_lml_kinv_batched_work_bytes(n, 1, 1) + lib.gpn_laplace_grad_batched_work_bytes(n, nls, 1)
        assert el.per_model_bytes(n, nls) == want > 2 * 8 * n * n          # at least the factor and B^-1


def _oracle(case, inp, variance, ell, **search):
    base = np.atleast_1d(np.asarray(case["length_scales"], dtype=np.float64))
    return eo.build_oracle(dict(case, variance=variance, length_scales=list(base * 0 + ell)), inp).search(**search)


def test_the_gpu_tests_searches_differ_in_length_and_one_stalls():
    """conditions on the INPUTS of tests/test_gpu_ep_lockstep.py, by the CPU oracle: the three settings sweep a different number of
    times each (so models leave the lock-step search one after the other), and ep_tol = 0 ends by the stall rule (or with a change
    of exactly zero) within max_sweeps."""
    for name in ("probit_rbf_300x2", "logit_matern52_300x3"):
        case = CASES[name]
        inp = lo.case_inputs(case)
        sweeps = [_oracle(case, inp, v, ell).sweeps for v, ell in SETTINGS]
        print("%s: oracle sweeps %s" % (name, sweeps))
        assert len(set(sweeps)) == 3, sweeps
    case = CASES["probit_rbf_300x2"]
    o = _oracle(case, lo.case_inputs(case), *SETTINGS[1], tol=0.0)
    print("ep_tol = 0: oracle sweeps %d stalled %s" % (o.sweeps, o.stalled))
    assert o.stalled and o.sweeps < 200
