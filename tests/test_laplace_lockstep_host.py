"""LaplaceGP in lock step, the part that needs no GPU: the new entry points are declared, exported and bound, they validate their
arguments before any launch, their workspaces are `batch` times the single ones, and the grouping keeps apart what must not share
a call."""
import ctypes
import os
import re

import numpy as np
import torch

from gptorch_amd import _native, _ops, kernels, likelihoods, rng
from gptorch_amd.models import GPR, VFE, LaplaceGP
from gptorch_amd.models import _laplace_lockstep as ll
from gptorch_amd.models import _lockstep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gpn_lik_derivs_batched_work_bytes", "gpn_lik_derivs_batched", "gpn_laplace_system_batched", "gpn_laplace_rows_batched_work_bytes",
       "gpn_laplace_matvec_batched", "gpn_laplace_diag_batched", "gpn_laplace_grad_batched_work_bytes", "gpn_laplace_grad_batched",
       "gpn_backsub_batched_work_bytes", "gpn_backsub_batched"]
UNSUPPORTED = -102
P = ctypes.c_void_p(64)         # a non-null "pointer": every call below returns before anything could follow it


def test_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpnative.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gpn_\w+)\s*\(", text))
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
    for name in ("lik_derivs_batched", "laplace_system_batched", "laplace_matvec_batched", "laplace_diag_batched", "laplace_grad_batched",
                 "backsub_batched"):
        assert callable(getattr(_ops, name)), name
    assert set(ll.STATS) == {"searches", "rounds", "trial_reads", "factorisations"}
    assert callable(ll.find_modes) and callable(ll.supported) and callable(ll.per_model_bytes)
    assert issubclass(ll.BatchedLaplaceEvidence, torch.autograd.Function)


def test_argument_validation_without_launch():
    """-(argument index), the stream being argument 1, before any HIP call; a batch beyond a grid dimension: GPN_E_UNSUPPORTED"""
    lib = _native.lib()
    null = None
    # gpn_lik_derivs_batched(stream, kind, batch, f, sf, y, sy, n, work, work_bytes, value, d1, w, d3)
    assert lib.gpn_lik_derivs_batched(null, 7, 2, null, 0, null, 0, 4, null, 0, null, null, null, null) == -2
    assert lib.gpn_lik_derivs_batched(null, _native.LIK_STUDENT_T, 2, null, 0, null, 0, 4, null, 0, null, null, null, null) == UNSUPPORTED
    assert lib.gpn_lik_derivs_batched(null, 0, 0, null, 0, null, 0, 4, null, 0, null, null, null, null) == -3
    assert lib.gpn_lik_derivs_batched(null, 0, 2, null, 0, null, 0, 4, null, 0, null, null, null, null) == -4
    assert lib.gpn_lik_derivs_batched(null, 0, 2, P, -1, null, 0, 4, null, 0, null, null, null, null) == -5
    assert lib.gpn_lik_derivs_batched(null, 0, 2, P, 4, null, 0, 4, null, 0, null, null, null, null) == -6
    assert lib.gpn_lik_derivs_batched(null, 0, 2, P, 4, P, 0, 0, null, 0, null, null, null, null) == -8
    assert lib.gpn_lik_derivs_batched(null, 0, 2, P, 4, P, 0, 4, null, 0, null, null, null, null) == -9
    assert lib.gpn_lik_derivs_batched(null, 0, 2, P, 4, P, 0, 4, P, 8, null, null, null, null) == -10
    assert lib.gpn_lik_derivs_batched(null, 0, 65536, P, 4, P, 0, 4, P, 1 << 30, null, null, null, null) == UNSUPPORTED
    # gpn_laplace_system_batched(stream, kind, batch, X, sX, n, d, variance, length_scales, nls, s, ss, A, lda, sA)
    assert lib.gpn_laplace_system_batched(null, 9, 2, null, 0, 4, 2, null, null, 1, null, 0, null, 128, 0) == -2
    assert lib.gpn_laplace_system_batched(null, 0, 0, null, 0, 4, 2, null, null, 1, null, 0, null, 128, 0) == -3
    assert lib.gpn_laplace_system_batched(null, 0, 2, null, 0, 4, 2, null, null, 1, null, 0, null, 128, 0) == -4
    assert lib.gpn_laplace_system_batched(null, 0, 2, P, -8, 4, 2, null, null, 1, null, 0, null, 128, 0) == -5
    assert lib.gpn_laplace_system_batched(null, 0, 2, P, 0, 4, 0, null, null, 1, null, 0, null, 128, 0) == -7
    assert lib.gpn_laplace_system_batched(null, 0, 2, P, 0, 4, 2, P, P, 3, null, 0, null, 128, 0) == -10
    assert lib.gpn_laplace_system_batched(null, 0, 2, P, 0, 4, 2, P, P, 1, null, 0, null, 128, 0) == -11
    assert lib.gpn_laplace_system_batched(null, 0, 2, P, 0, 4, 2, P, P, 1, P, 4, null, 128, 0) == -13
    assert lib.gpn_laplace_system_batched(null, 0, 2, P, 0, 4, 2, P, P, 1, P, 4, P, 3, 0) == -14
    assert lib.gpn_laplace_system_batched(null, 0, 2, P, 0, 4, 2, P, P, 1, P, 4, P, 128, 100) == -15        # slots would overlap
    assert lib.gpn_laplace_system_batched(null, 0, 65536, P, 0, 4, 2, P, P, 1, P, 4, P, 128, 1024) == UNSUPPORTED
    # gpn_laplace_matvec_batched(stream, kind, batch, X, sX, n, d, variance, length_scales, nls, v, sv, work, out)
    assert lib.gpn_laplace_matvec_batched(null, -1, 2, null, 0, 4, 2, null, null, 1, null, 0, null, null) == -2
    assert lib.gpn_laplace_matvec_batched(null, 1, 2, null, 0, 4, 2, null, null, 1, null, 0, null, null) == -4
    assert lib.gpn_laplace_matvec_batched(null, 1, 2, P, 0, 4, 2, P, P, 1, null, 0, null, null) == -11
    assert lib.gpn_laplace_matvec_batched(null, 1, 2, P, 0, 4, 2, P, P, 1, P, 4, null, null) == -13
    assert lib.gpn_laplace_matvec_batched(null, 1, 2, P, 0, 4, 2, P, P, 1, P, 4, P, null) == -14
    assert lib.gpn_laplace_matvec_batched(null, 1, 65536, P, 0, 4, 2, P, P, 1, P, 4, P, P) == UNSUPPORTED
    # gpn_laplace_diag_batched(stream, kind, batch, X, sX, n, d, variance, length_scales, nls, s, ss, Binv, ldb, sB, work, sigma)
    assert lib.gpn_laplace_diag_batched(null, 6, 2, null, 0, 4, 2, null, null, 1, null, 0, null, 4, 0, null, null) == -2
    assert lib.gpn_laplace_diag_batched(null, 0, 2, null, 0, 4, 2, null, null, 1, null, 0, null, 4, 0, null, null) == -4
    assert lib.gpn_laplace_diag_batched(null, 0, 2, P, 0, 4, 2, P, P, 1, P, 4, null, 4, 0, null, null) == -13
    assert lib.gpn_laplace_diag_batched(null, 0, 2, P, 0, 4, 2, P, P, 1, P, 4, P, 3, 0, null, null) == -14
    assert lib.gpn_laplace_diag_batched(null, 0, 2, P, 0, 4, 2, P, P, 1, P, 4, P, 4, 16, null, null) == -16
    assert lib.gpn_laplace_diag_batched(null, 0, 65536, P, 0, 4, 2, P, P, 1, P, 4, P, 4, 16, P, P) == UNSUPPORTED
    # gpn_laplace_grad_batched(stream, kind, batch, X, sX, n, d, variance, length_scales, nls, s, Binv, ldb, sB, a, u, d1, sv, work, out)
    assert lib.gpn_laplace_grad_batched(null, 6, 2, null, 0, 4, 2, null, null, 1, null, null, 4, 0, null, null, null, 0, null, null) == -2
    assert lib.gpn_laplace_grad_batched(null, 0, 2, null, 0, 4, 2, null, null, 1, null, null, 4, 0, null, null, null, 0, null, null) == -4
    assert lib.gpn_laplace_grad_batched(null, 0, 2, P, 0, 4, 2, P, P, 1, P, P, 3, 0, null, null, null, 0, null, null) == -13
    assert lib.gpn_laplace_grad_batched(null, 0, 2, P, 0, 4, 2, P, P, 1, P, P, 4, 16, P, P, null, 4, null, null) == -17
    assert lib.gpn_laplace_grad_batched(null, 0, 2, P, 0, 4, 2, P, P, 1, P, P, 4, 16, P, P, P, 4, P, null) == -20
    assert lib.gpn_laplace_grad_batched(null, 0, 65536, P, 0, 4, 2, P, P, 1, P, P, 4, 16, P, P, P, 4, P, P) == UNSUPPORTED
    # gpn_backsub_batched(stream, batch, A, lda, sA, winv, sW, n, dy, work, out, ldo, so)
    assert lib.gpn_backsub_batched(null, 0, null, 128, 0, null, 0, 4, 1, null, null, 4, 4) == -2
    assert lib.gpn_backsub_batched(null, 2, null, 128, 0, null, 0, 4, 1, null, null, 4, 4) == -3
    assert lib.gpn_backsub_batched(null, 2, P, 100, 0, null, 0, 4, 1, null, null, 4, 4) == -4
    assert lib.gpn_backsub_batched(null, 2, P, 128, 0, null, 0, 4, 1, null, null, 4, 4) == -5
    sa, sw = 144 * 128, 128 * 128
    assert lib.gpn_backsub_batched(null, 2, P, 128, sa, null, sw, 4, 1, null, null, 4, 4) == -6
    assert lib.gpn_backsub_batched(null, 2, P, 128, sa, P, 5, 4, 1, null, null, 4, 4) == -7
    assert lib.gpn_backsub_batched(null, 2, P, 128, sa, P, sw, 4, 0, null, null, 4, 4) == -9
    assert lib.gpn_backsub_batched(null, 2, P, 128, sa, P, sw, 4, 1, null, null, 4, 4) == -10
    assert lib.gpn_backsub_batched(null, 2, P, 128, sa, P, sw, 4, 1, P, P, 3, 4) == -12
    assert lib.gpn_backsub_batched(null, 2, P, 128, sa, P, sw, 4, 1, P, P, 4, 3) == -13
    assert lib.gpn_backsub_batched(null, 65536, P, 128, sa, P, sw, 4, 1, P, P, 4, 4) == UNSUPPORTED


def test_workspaces_are_batch_times_the_single_ones():
    lib = _native.lib()
    for n in (1, 256, 257, 300, 5000):
        for batch in (1, 3, 64):
            assert lib.gpn_lik_derivs_batched_work_bytes(n, batch) == batch * lib.gpn_lik_derivs_work_bytes(n)
            assert lib.gpn_laplace_rows_batched_work_bytes(n, batch) == batch * lib.gpn_laplace_rows_work_bytes(n)
            assert lib.gpn_backsub_batched_work_bytes(n, 1, batch) == batch * lib.gpn_backsub_work_bytes(n, 1)
            assert lib.gpn_backsub_batched_work_bytes(n, 3, batch) == batch * lib.gpn_backsub_work_bytes(n, 3)
            for nls in (1, 5):
                assert lib.gpn_laplace_grad_batched_work_bytes(n, nls, batch) == batch * lib.gpn_laplace_grad_work_bytes(n, nls)
    assert lib.gpn_lik_derivs_batched_work_bytes(300, 0) == 0 and lib.gpn_laplace_rows_batched_work_bytes(0, 4) == 0
    assert lib.gpn_laplace_grad_batched_work_bytes(300, 1, -1) == 0 and lib.gpn_backsub_batched_work_bytes(300, 0, 4) == 0


def _laplace(n, kernel, lik, seed=1):
    x = rng.normal(seed, (n, 2))
    y = (rng.uniform(seed + 1, n) < 0.5).astype(np.float64).reshape(n, 1)
    return LaplaceGP(x, y, kernel, lik)


def test_grouping_on_the_host():
    base = [_laplace(30, kernels.Rbf(2), likelihoods.Bernoulli("probit"), seed=s) for s in (1, 2)]
    assert _lockstep._laplace_groups(base) == []                          # CPU-resident models: nothing to run in lock step
    assert _lockstep._laplace_key(base[0]) == _lockstep._laplace_key(base[1])
    others = [_laplace(30, kernels.Rbf(2), likelihoods.Bernoulli("logit")),            # likelihood kind
              _laplace(30, kernels.Rbf(2), likelihoods.Poisson()),
              _laplace(30, kernels.Matern52(2), likelihoods.Bernoulli("probit")),      # kernel kind
              _laplace(30, kernels.Rbf(2, ARD=True), likelihoods.Bernoulli("probit")),  # ARD
              _laplace(31, kernels.Rbf(2), likelihoods.Bernoulli("probit"))]           # N
    keys = [_lockstep._laplace_key(m) for m in [base[0]] + others]
    assert len(set(keys)) == len(keys)
    assert ll.supported(1) and ll.supported(512) and not ll.supported(0)
    assert ll.per_model_bytes(300) == 3 * 8 * (512 + 16) * 512              # three padded N x N matrices, as for a GPR model
    # a GPR / VFE list with the CPU-resident LaplaceGP models: the plan is what every family takes from it, one after the other,
    # each group with its priors flag -- and it holds no laplace or ep group
    x, y = rng.make_regression(40, 2, 1, seed=3)
    ms = [GPR(x, y, kernels.Rbf(2)) for _ in range(2)] + [VFE(x, y, kernels.Rbf(2), inducing_points=x[:8]) for _ in range(2)]
    plan = _lockstep._plan_groups(ms + base)
    assert plan == [grp._replace(priors=_lockstep._has_priors([(ms + base)[i] for i in grp.indices]))
                    for family in _lockstep.FAMILIES for grp in family.groups(ms + base)]
    assert not [grp for grp in plan if grp.family.name in ("laplace", "ep")]
