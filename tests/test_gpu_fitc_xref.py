"""The streamed FITC likelihood, its closed-form backward and its predictions (gptorch_amd/models/_fitc.py, csrc/fitc.hip, on the
pipeline of sparse_gpr._stream_gram) against the long-double statement tests/_sparse_ref.FITCRef, on every route the switches of
gptorch_amd/models/sparse_gpr.py select -- chunk size, one or two lanes, split-K partials and the chunks that miss the split, short
K slices, the blocked right-solve, the jitter ladder, a composite kernel through the autograd adapter -- at the smallest shapes that
cross each switch's edge (tests/_sparse_ref.FITC_CASES).  A quarter of Z lies on rows of x: there lambda_i = noise after the
cancellation of Kdiag - |a_i|^2.

Tolerances are tests/_xref.tol: max(16 e64, FLOOR[what]), e64 the distance of the plain fp64 CPU evaluation of the same quantity
(tests/_sparse_ref.Direct64FITC, the M-sized Woodbury form with autograd gradients) from the long-double one;
tests/test_fitc_ref_host.py checks the reference itself, holds every tolerance under the fixed one the suite used before, and shows
that each of five planted mistakes (a row lost from B, a chunk's slot of the scalar sums lost, A diag(g) A^T not mirrored, the Kdiag
pull-back dropped, g without its h term) lies at least 100 tolerances from the reference on a case run here.  Loss and gradients are
relative to max(1, |reference|) (xr.rel_err), predictions absolute.  Every check prints achieved error against tolerance (pytest -s).

Measured on an MI355X (achieved / tolerance; "grad": the parameter block with the least margin).  Except for inverse_knob_ignored's
d/dZ and the ladder case 16 e64 is below the floors, so those are the tolerances: 1e-10 loss, 1e-9 gradients, 1e-10 predictions.

    case (knobs)                                  loss            gradient, least margin                 mean      var
    one_chunk                                     5.5e-15         5.6e-14  Z                             2.3e-15   4.8e-16
    m_odd_across_a_leaf                           3.1e-15         7.9e-13  mean                          2.1e-14   1.8e-15
    dy_across_16                                  1.1e-16         1.4e-13  Z                             4.7e-15   1.6e-15
    ragged_multi_chunk (LANES 1 and 2: same bits) 3.1e-15         8.5e-13  Z                             1.1e-14   9.7e-15
    exact_multiple                                2.3e-15         2.8e-13  Z                             3.9e-15   1.8e-15
    short_k_slices (128 / 0)                      1.6e-15         2.2e-13 / 4.0e-13  Z                   6.9e-15   2.3e-15
    split_k_tail                                  3.1e-15         1.2e-13  Z                             6.9e-14   2.1e-15
    split_k_miss (one chunk / 8192 + 8)           1.2e-14/1.6e-14 1.7e-12 / 7.5e-13  Z                   6.3e-14   1.4e-15
    blocked_one_block                             4.8e-18         1.1e-13  Z                             4.9e-15   2.1e-15
    blocked_two_blocks                            1.4e-14         2.7e-11  Z (37x)                       1.2e-13   4.4e-15
    composite (LANES 1 and 2: same bits)          8.3e-15         7.8e-13  Constant's variance           2.6e-14   2.7e-14
    inverse_knob_ignored                          4.0e-12         4.0e-9/1.3e-8  Z (3.2x)                7.5e-12   1.0e-11
    ladder (rung 0)                               1.5e-10/7.0e-10 (not judged; Z 3.9e-8 of 2.0e-7)       3.4e-11   1.0e-10/5e-10
    one_chunk on 192 gathered rows                4.1e-15         7.3e-15  Z                             -         -

No route has less than twice its tolerance in hand.  The least margins: inverse_knob_ignored's d/dZ, 3.2x of a tolerance that is
16 e64 itself (cond K(Z) = 1.3e8 there; e64 of that block was 8e-10 on the machine of this run and 2.2e-9 on another, the order of
fp64 sums in the CPU evaluation moves it), the ladder case's loss and variance at 4.6x / 5x, and blocked_two_blocks' d/dZ at 37x.
Where a case has two knob sets the two runs differ by at most 2.4e-12 (split_k_miss, d/dZ; short_k_slices: 2.4e-13).
"""
import functools

import numpy as np
import pytest
import torch

from gptorch_amd import _ops
from gptorch_amd.models import sparse_gpr
from tests import _fitc_oracle as fo
from tests import _sparse_ref as sr
from tests import _xref as xr
from tests._util import load_json
from tests.test_gpu_sparse_xref import KNOBS, assert_route, check_grads, check_loss, check_predictions

pytestmark = pytest.mark.gpu

LD = xr.LD
CASES = {c["name"]: c for c in sr.FITC_CASES}
ROUTED = [c for c in sr.FITC_CASES if not c.get("ladder")]


@functools.lru_cache(maxsize=None)
def inputs(name):
    return sr.case_inputs(CASES[name])


@functools.lru_cache(maxsize=None)
def reference(name, jitter=0.0):
    """computed once per module and left as it is; the case that is too large for that comes from its fixture
    (tests/golden/make_sparse_xref_golden.py)."""
    case = CASES[name]
    if case.get("golden"):
        g = {c["name"]: c for c in load_json("fitc_xref_cases.json")["cases"]}[name]
        assert all(g[k] == case[k] for k in ("n", "m", "d", "dy", "kernel", "noise", "seed"))
        return dict(loss=g["loss"], grads=g["grads"], mean=g["mean_pred"], var=g["var_pred"], cov=g["cov_pred"], e64=g["e64"])
    return sr.fitc_reference(case, inputs(name), jitter)


def fitc_model(case, inp):
    m = fo.build_model(case, inp)
    m.cuda()
    return m


def grads_of(m, names):
    params = dict(m.named_parameters())
    return {mn: params[mn].grad.detach().cpu().numpy().copy() for mn in names.values()}


@pytest.mark.parametrize("case", ROUTED, ids=[c["name"] for c in ROUTED])
def test_fitc(device, monkeypatch, case):
    """loss, every parameter gradient (Z, the noise and the mean included), predict_f (diag and full) and predict_y's variance, once
    per knob set of the case, each against the one reference of the case; two knob sets also agree with each other within the same
    tolerances, and under two lanes a second loss(); backward() gives the bits of the first."""
    inp, ref = inputs(case["name"]), reference(case["name"])
    names, runs = fo.model_names(case), []
    assert ("mean" in names) == ("mean" in case)
    for knobs in case["knobs"]:
        with monkeypatch.context() as mp:
            for k, v in knobs.items():
                assert k in KNOBS
                mp.setattr(sparse_gpr, k, v)
            assert_route(case, knobs)
            inverse_calls, lower_inverse = [], _ops.lower_inverse
            mp.setattr(_ops, "lower_inverse", lambda f: (inverse_calls.append(1), lower_inverse(f))[1])
            m = fitc_model(case, inp)
            loss = m.loss()
            loss.backward()
            assert not inverse_calls                                       # a hooked evaluation never takes the inverse form
            check_loss("fitc/%s %s" % (case["name"], knobs or "defaults"), loss, ref)
            check_grads(m, names, ref)
            check_predictions(m, inp, ref, case["noise"])
            runs.append((loss.item(), grads_of(m, names)))
            if case["name"] == "ragged_multi_chunk" and knobs.get("LANES") == 2:
                m.zero_grad()
                again = m.loss()
                again.backward()
                assert again.item() == loss.item()
                for mn, g in grads_of(m, names).items():
                    assert np.array_equal(g, runs[-1][1][mn]), mn
    for (la, ga), (lb, gb) in zip(runs, runs[1:]):
        assert xr.rel_err(la, lb) <= xr.tol(ref["e64"]["loss"], "loss")
        for on, mn in names.items():
            err = xr.rel_err(ga[mn], gb[mn])
            print("   first against second knob set d/d%-24s rel diff %.2e" % (mn, err))
            assert err <= xr.tol(ref["e64"]["grads"][on], "grad"), mn


def test_fitc_ladder(device):
    """two identical inducing points: K(Z) is singular, the native factorisation climbs the jitter ladder and reports its rung; the
    reference is given that jitter, 10^(-10 + rung).  The likelihood and predict_f are judged, at tolerances that are printed (cond
    K(Z) ~ 1e11); the gradients are printed against theirs."""
    case, inp = CASES["ladder"], inputs("ladder")
    assert np.array_equal(inp["z"][-1], inp["z"][-2])
    m = fitc_model(case, inp)
    loss = m.loss()
    loss.backward()
    rung = m._state_for_predict(m.X).f_uu.jitter_rung
    print("fitc/ladder: rung %d" % rung)
    assert rung >= 0
    ref = reference("ladder", 10.0 ** (-10 + rung))
    check_loss("fitc/ladder", loss, ref)
    check_predictions(m, inp, ref, case["noise"])
    params = dict(m.named_parameters())
    for on, mn in fo.model_names(case).items():
        print("   (not judged) d/d%-19s rel err %.2e (tol %.1e)" % (mn, xr.rel_err(params[mn].grad.cpu().numpy(), np.asarray(ref["grads"][on], dtype=LD).reshape(params[mn].shape)),
                                                              xr.tol(ref["e64"]["grads"][on], "grad")))


def test_fitc_on_gathered_rows(device):
    """log_likelihood(x=X[i], y=Y[i]) on a sorted index set of 192 of one_chunk's 300 rows that is no slice (the row kernels read what
    _ops._c makes of the gathered rows), and its gradients, against a FITCRef built on those rows."""
    case, inp = CASES["one_chunk"], inputs("one_chunk")
    idx = np.sort(np.random.RandomState(case["seed"]).choice(case["n"], 192, replace=False))
    assert len(idx) == 192 and bool((np.diff(idx) > 1).any()) and bool((np.diff(idx) > 0).all())
    rows = dict(inp, x=inp["x"][idx], y=inp["y"][idx])
    ref = sr.fitc_reference(case, rows)
    m = fitc_model(case, inp)
    i = torch.as_tensor(idx, device=m.X.device)
    ll = m.log_likelihood(x=m.X[i], y=m.Y[i])
    (-ll).backward()
    check_loss("fitc/one_chunk on 192 gathered rows", -ll, ref)
    check_grads(m, fo.model_names(case), ref)
