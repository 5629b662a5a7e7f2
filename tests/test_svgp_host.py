"""SVGP on the host (no GPU): the oracle against the goldens, construction and _init_posterior on a CPU-resident model, the
minibatch rule's use of np.random, error paths, argument validation of the gpn_svgp_* entry points, parameter names."""
import numpy as np
import pytest
import torch

from gptorch_amd import _native, kernels, likelihoods, mean_functions
from gptorch_amd.models import SVGP
from tests import _svgp_oracle as so
from tests._util import load_json, load_npz

CASES = load_json("svgp_cases.json")


def golden_grad(entry, arrays, shape):
    """a gradient block of svgp_cases.json: inline list, or "npz:<key>" (the Cholesky factor's block packed as its lower triangle)."""
    if isinstance(entry, str):
        a = arrays[entry[4:]]
        if a.ndim == 1 and len(shape) == 2 and shape[0] == shape[1] and a.size == shape[0] * (shape[0] + 1) // 2:
            full = np.zeros(shape)
            full[np.tril_indices(shape[0])] = a
            return full
        return a.reshape(shape)
    return np.asarray(entry, dtype=np.float64).reshape(shape)


def inputs_of(case, arrays):
    return so.case_inputs(case, z=arrays["wellcond.z"] if case["name"].startswith("wellcond") else None)


@pytest.mark.parametrize("case", CASES["cases"], ids=[c["name"] for c in CASES["cases"]])
def test_oracle_reproduces_golden(case):
    arrays = load_npz("svgp_cases.npz")
    inp = inputs_of(case, arrays)
    names = so.model_names(case)
    for ev in case["evals"]:
        o = so.oracle_for(case, inp)
        loss, grads = o.loss_and_grads(idx=inp["idx"] if ev["tag"] == "batch" else None)
        assert abs(loss - ev["loss"]) < 1e-9 * abs(ev["loss"])
        for on, mn in names.items():
            want = golden_grad(ev["grads"][mn], arrays, grads[on].shape)
            assert np.max(np.abs(grads[on] - want)) < 1e-8 * np.max(np.abs(want)), mn
    o = so.oracle_for(case, inp)
    mu, var = o.predict_f(inp["xs"])
    _, cov = o.predict_f(inp["xs"], diag=False)
    assert np.max(np.abs(mu - np.asarray(case["mean_pred"]))) < 1e-9
    assert np.max(np.abs(var - np.asarray(case["var_pred"]))) < 1e-9
    assert np.max(np.abs(cov - np.asarray(case["cov_pred"]))) < 1e-9


def test_oracle_reproduces_trajectory():
    t = CASES["trajectory"]
    inp = so.case_inputs(t)
    o = so.oracle_for(t, inp, batch_size=t["batch_size"])
    np.random.seed(t["np_seed"])
    losses = o.optimize_adam(t["steps"], t["learning_rate"])
    assert np.max(np.abs(np.asarray(losses) - np.asarray(t["losses"])) / np.maximum(1.0, np.abs(t["losses"]))) < 1e-9


def _xyz():
    f = load_npz("ref_sparse_gpr_fixtures.npz")
    return f["x"], f["y"], f["z"]


def test_constructor_forms_on_the_host():
    """test/test_models/test_sparse_gpr.py:180-192."""
    x, y, z = _xyz()
    kernel = kernels.Matern32(x.shape[1], ARD=True)
    SVGP(x, y, kernel)
    SVGP(x, y, kernel, inducing_points=z)
    SVGP(x, y, kernel, mean_function=mean_functions.Constant(y.shape[1]))
    m = SVGP(x, y, kernel, mean_function=torch.nn.Linear(x.shape[1], y.shape[1], dtype=torch.float64))
    assert not m.X.is_cuda and m.batch_size is None
    assert isinstance(m.likelihood, likelihoods.Gaussian) and m.likelihood.variance.transform().item() == pytest.approx(1.0)


def test_init_posterior_equals_the_reference_under_a_seed():
    c = CASES["init"]
    inp = so.case_inputs(c)
    np.random.seed(c["np_seed"])
    m = SVGP(inp["x"], inp["y"], kernels.Matern52(c["d"], variance=1.3, length_scales=1.2), inducing_points=inp["z"].copy(),
             likelihood=likelihoods.Gaussian(variance=c["noise"]),
             mean_function=mean_functions.Constant(2, val=torch.tensor(c["mean"], dtype=torch.float64)))
    assert int(np.random.permutation(1000)[0]) == c["next_draw"]            # exactly one permutation consumed
    want_m, want_s = np.asarray(c["induced_output_mean"]), np.asarray(c["induced_output_chol_cov"])
    assert np.max(np.abs(m.induced_output_mean.detach().numpy() - want_m)) < 1e-9 * max(1.0, np.max(np.abs(want_m)))
    assert np.max(np.abs(m.induced_output_chol_cov.transform().detach().numpy() - want_s)) < 1e-9 * max(1.0, np.max(np.abs(want_s)))


def test_parameter_names():
    x, y, z = _xyz()
    m = SVGP(x, y, kernels.Matern32(1), inducing_points=z, mean_function=mean_functions.Constant(1))
    assert set(m.state_dict()) == {"Z", "induced_output_mean", "induced_output_chol_cov", "kernel.variance", "kernel.length_scales",
                                   "likelihood.variance", "mean_function.val"}
    assert tuple(m.induced_output_mean.shape) == (z.shape[0], 1) and tuple(m.induced_output_chol_cov.shape) == (z.shape[0],) * 2
    S = m.induced_output_chol_cov.transform()
    assert torch.equal(S, S.tril()) and bool((S.diagonal() > 0).all())


def test_minibatch_rule_draws_like_the_reference(monkeypatch):
    """sparse_gpr.py:198-216: one np.random.permutation(num_data)[:batch_size] per evaluation, none when (x, y) are given."""
    x, y = np.arange(40.0)[:, None] * np.ones((1, 2)), np.arange(40.0)[:, None]
    m = SVGP(x, y, kernels.Rbf(2), inducing_points=x[::10].copy(), batch_size=7)
    seen = []

    def fake(self, xb):
        seen.append(xb[:, 0].numpy().copy())
        return torch.zeros(xb.shape[0], 1, dtype=torch.float64), torch.ones(xb.shape[0], dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    monkeypatch.setattr(SVGP, "_marginals", fake)
    np.random.seed(5)
    m.log_likelihood(), m.log_likelihood()
    rs = np.random.RandomState(5)
    want = [rs.permutation(40)[:7].astype(np.float64) for _ in range(2)]
    assert all(np.array_equal(a, b) for a, b in zip(seen, want))
    assert np.random.permutation(1000)[0] == rs.permutation(1000)[0]        # two draws, no more
    np.random.seed(6)
    out = m.log_likelihood(torch.tensor(x[:5]), torch.tensor(y[:5]))
    assert out.dim() == 0 and seen[-1].shape == (5,)
    assert np.random.permutation(1000)[0] == np.random.RandomState(6).permutation(1000)[0]   # explicit (x, y): no draw
    m.batch_size = None
    m.log_likelihood()
    assert seen[-1].shape == (40,)


def test_error_paths(monkeypatch):
    x, y, z = _xyz()
    m = SVGP(x, y, kernels.Matern32(1), inducing_points=z)
    with pytest.raises(ValueError, match="X and Y must have same # data."):
        m.log_likelihood(torch.tensor(x[: x.shape[0] // 2]), torch.tensor(y))
    with pytest.raises(ValueError, match="y is required"):
        m.log_likelihood(torch.tensor(x))
    with pytest.raises(_native.NativeError):                                # no CPU arithmetic behind the bound
        m.log_likelihood()
    assert not m._can_capture("Adam")


def test_svgp_entry_points_validate_without_launch():
    lib = _native.lib()
    n = None
    one = 1 << 4                                                            # any non-null, 16-byte aligned address: nothing is launched
    ok = dict(alpha=one, lda=16, T=one, ldt=16, rows=4, m=10, w=one, ldw=2, dy=2)

    def marg(**kw):
        a = dict(ok, kdiag=one, kds=0, f_mean=one, f_var=one)
        a.update(kw)
        return lib.gpn_svgp_marginals(n, a["alpha"], a["lda"], a["T"], a["ldt"], a["rows"], a["m"], a["w"], a["ldw"], a["dy"], a["kdiag"],
                                      a["kds"], a["f_mean"], a["f_var"])

    def rows(**kw):
        a = dict(ok, g_var=one, g_mean=one, aT=one, gaT=one, ldo=16)
        a.update(kw)
        return lib.gpn_svgp_backward_rows(n, a["alpha"], a["lda"], a["T"], a["ldt"], a["rows"], a["m"], a["w"], a["ldw"], a["dy"], a["g_var"],
                                          a["g_mean"], a["aT"], a["gaT"], a["ldo"])
    for f in (marg, rows):
        assert f(alpha=None) == -2 and f(lda=8) == -3 and f(T=None) == -4 and f(ldt=9) == -5
        assert f(rows=0) == -6 and f(m=0) == -7 and f(w=None) == -8 and f(ldw=1) == -9 and f(dy=0) == -10
        assert f(lda=17) == -101 and f(alpha=one + 8) == -101
    assert marg(kdiag=None) == -11 and marg(kds=-1) == -12 and marg(f_mean=None) == -13 and marg(f_var=None) == -14
    assert rows(g_var=None) == -11 and rows(g_mean=None) == -12 and rows(aT=None) == -13 and rows(gaT=None) == -14
    assert rows(ldo=15) == -15 and rows(rows=17, ldo=16) == -15 and rows(ldo=17, rows=1) == -101
