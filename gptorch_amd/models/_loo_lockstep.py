"""
Leave-one-out GPR models in lock step: which sizes take the lock-step route and what one model of a group holds on the device.
The node itself is _ops.BatchedGPRLooLik (beside GPRLooLik, whose launches it issues once over the group); the grouping is
_lockstep._loo_groups.
"""
from .. import _native, _ops

# supported() admits 1 <= n <= MAX_N.  MAX_N is the largest MEASURED size at which the lock-step [min, max] of batched_loss_and_grad
# lies entirely below the parent commit's (tools/loo_lockstep_bench.py, profiles/loo_lockstep.json, LAB 25): all three measured
# shapes -- 512 x 64, 2048 x 16, 8192 x 8 -- clear that bar, so MAX_N is the largest of them.  Nothing was measured beyond it, so
# nothing beyond it is admitted: such models keep their own loss(), one after the other.
MAX_N = 8192


def supported(n):
    return 1 <= int(n) <= MAX_N


def per_model_bytes(n, dy, nls):
    """device bytes ONE model of a lock-step LOO group holds at the peak (the backward), from the library's own size functions: its
    factor slot (+ the leaf inverses), gpn_lml_kinv_batched's block (U -- later S --, P, a^T), Q, the right-hand-side buffer of w, the
    sweep's and the terms' partial sums, and the per-point vectors (w^T, 1 / p, sqrt d).  Four padded N x N matrices and change."""
    lib = _native.lib()
    n, dy, nls = int(n), int(dy), int(nls)
    ld = int(lib.gpn_factor_ld(n, dy))
    factor = 8 * int(lib.gpn_factor_rows(n, dy)) * ld + max(16, int(lib.gpn_winv_bytes(n)))
    kinv = int(lib.gpn_lml_kinv_batched_work_bytes(n, dy, 1))
    q = 8 * _ops.round_up(max(n, 1), 64) * int(lib.gpn_factor_ld(n, 0))
    rhs = 8 * _ops.round_up(max(dy, 1), _ops.LEAF) * ld
    partials = int(lib.gpn_loo_grad_batched_work_bytes(n, nls, 1)) + int(lib.gpn_loo_terms_batched_work_bytes(n, 1))
    vectors = 8 * (dy * n + 2 * n)
    return factor + kinv + q + rhs + partials + vectors
