"""The row kernels' long-double reference (tests/_rowref.py) on the host, no GPU: its four statements, composed with dense
matmuls into the quantities of the two host oracles on a small case (N = 60, M = 13, dy = 3), agree with tests/_fitc_oracle.py
(lambda, the scalar sums and the likelihood they give, r, g, dF/dA^T) and tests/_svgp_oracle.py (the marginals of q(f), and the
backward's G_alpha and transposed operands against autograd) to 1e-12 -- two host statements of the same thing --, in long double
and in the float64 form the GPU tests' tolerances come from."""
import math

import numpy as np
import pytest
import torch

from gptorch_amd import rng
from oracle import gp_oracle as orc
from tests import _fitc_oracle as fo
from tests import _rowref as rr
from tests import _svgp_oracle as so
from tests import _xref as xr

N, M, D, DY = 60, 13, 2, 3
TOL = 1e-12
DTYPES = [rr.LD, np.float64]


def _data():
    x, y = rng.make_regression(N, D, DY, seed=71)
    z = x[:: N // M][:M] + 0.05 * rng.normal(72, (M, D))                     # no coincident points: an ordinary lambda
    return x, y, z


@pytest.fixture(scope="module")
def fitc():
    """the quantities of FITCOracle.closed_form_check / woodbury_lml, in fp64 torch, and autograd through the dense form."""
    x, y, z = _data()
    o = fo.FITCOracle(x, y, z, dict(kind="Matern52", variance=1.2, length_scales=1.1), 0.1)
    with torch.no_grad():
        leaves = [t.detach().clone().requires_grad_(True) for t in o._inputs()]
    F = o.dense_lml(*leaves)
    auto = torch.autograd.grad(F, leaves)
    Kuu, Kuf, Kd, s2, err = [t.detach() for t in leaves]
    L = torch.linalg.cholesky(Kuu)
    A = orc.trtrs(Kuf, L)
    lam = Kd - A.pow(2).sum(0) + s2
    B = torch.eye(M, dtype=torch.float64) + (A / lam) @ A.t()
    Binv = torch.linalg.inv(B)
    beta = Binv @ ((A / lam) @ err)
    r = (err - A.t() @ beta) / lam[:, None]
    g = r.pow(2).sum(1) - DY * (1.0 / lam - ((Binv @ A) * A).sum(0) / lam ** 2)
    dA = beta @ r.t() - DY * (Binv @ A) / lam - A * g
    n = lambda t: t.numpy().copy()
    return dict(o=o, F=F.item(), woodbury=o.woodbury_lml(Kuu, Kuf, Kd, s2, err).item(), auto=[n(a) for a in auto], L=n(L), A=n(A), Kd=n(Kd),
                s2=float(s2), err=n(err), lam=n(lam), B=n(B), Binv=n(Binv), beta=n(beta), r=n(r), g=n(g), dA=n(dA))


@pytest.mark.parametrize("dtype", DTYPES, ids=["long_double", "float64"])
def test_fitc_rows_compose_to_the_oracles_quantities(fitc, dtype):
    q = fitc
    alpha = q["A"].T.copy()                                                  # A_c^T = K(x, Z) L^-T [N, M]
    fwd = rr.fitc_forward_rows(alpha, q["err"], q["Kd"], q["s2"], dtype)
    assert fwd["lam"].dtype == dtype and xr.rel_err(fwd["lam"], q["lam"]) < TOL
    assert xr.rel_err(fwd["out2"][0], np.log(q["lam"]).sum()) < TOL
    assert xr.rel_err(fwd["out2"][1], (q["err"] ** 2 / q["lam"][:, None]).sum()) < TOL
    # the scaled rows and the scaled residual are the operands of B = I + A D A^T and b = A D err ...
    B = np.eye(M, dtype=dtype) + fwd["At"].T @ fwd["At"]
    b = fwd["At"].T @ fwd["errT"].T
    assert xr.rel_err(B, q["B"]) < TOL and xr.rel_err(b, q["B"] @ q["beta"]) < TOL
    # ... and with the two sums that is the Woodbury likelihood, which is the dense one
    LB = xr.cholesky(B)
    c = xr.solve_lower(LB, b)
    lml = -0.5 * DY * N * math.log(2.0 * math.pi) - 0.5 * DY * fwd["out2"][0] - DY * np.sum(np.log(np.diag(LB))) - 0.5 * fwd["out2"][1] \
        + 0.5 * np.sum(c * c)
    print("fitc lml from the row reference %.15f woodbury %.15f dense %.15f" % (float(lml), q["woodbury"], q["F"]))
    assert xr.rel_err(lml, q["woodbury"]) < TOL and xr.rel_err(lml, q["F"]) < TOL
    # backward: T = alpha [B^-1 | beta] is an input, the alpha beta block included
    mp = rr.round_up(M, 16)
    T = np.full((N, mp + DY + 1), 1e300)                                     # what lies between and behind the blocks is not read
    T[:, :M] = alpha @ q["Binv"]
    T[:, mp:mp + DY] = alpha @ q["beta"]
    bwd = rr.fitc_backward_rows(alpha, T, M, q["beta"], q["err"], q["lam"], dtype)
    assert xr.rel_err(bwd["r"], q["r"]) < TOL and xr.rel_err(bwd["g"], q["g"]) < TOL and xr.rel_err(bwd["T"], q["dA"].T) < TOL
    assert np.array_equal(bwd["alphaT"], q["A"].astype(dtype)) and xr.rel_err(bwd["galphaT"], q["A"] * q["g"]) < TOL
    # ... against autograd through the dense N x N form: dF/dKuf = U dF/dA, dF/dKdiag = g / 2, dF/derr = -r, and
    # dF/dKuu = -1/2 U S U^T with S = beta beta^T - p (I - B^-1) - A diag(g) A^T from the two transposed operands
    U = np.linalg.inv(q["L"]).T
    S = q["beta"] @ q["beta"].T - DY * (np.eye(M) - q["Binv"]) - np.asarray(bwd["galphaT"] @ bwd["alphaT"].T, dtype=np.float64)
    a_uu, a_uf, a_kd, _, a_err = q["auto"]
    assert xr.rel_err(U @ np.asarray(bwd["T"], dtype=np.float64).T, a_uf) < TOL
    assert xr.rel_err(0.5 * bwd["g"], a_kd) < TOL and xr.rel_err(-bwd["r"], a_err) < TOL
    assert xr.rel_err(-0.5 * U @ S @ U.T, 0.5 * (a_uu + a_uu.T)) < TOL
    assert fitc["o"].closed_form_check() < TOL


@pytest.fixture(scope="module")
def svgp():
    case = dict(n=N, d=D, dy=DY, m=M, kernel=dict(kind="Matern52", variance=1.2, length_scales=1.1), noise=0.1, seed_x=71, seed_z=72,
                seed_q=73, seed_xs=74)
    inp = so.case_inputs(case)
    o = so.oracle_for(case, inp)
    with torch.no_grad():
        L, S_L = o._factors()
        alpha = orc.trtrs(o.K(o.raw["Z"], o.X), L).t().contiguous()
        beta = orc.trtrs(S_L, L)
        Q = beta @ beta.t() - torch.eye(M, dtype=torch.float64)
        w = orc.trtrs(o.raw["q_mu"], L)
        kd = o.Kdiag(o.X).clone()
    return dict(o=o, L=L, alpha=alpha, Q=Q, w=w, kd=kd, g_var=torch.tensor(rng.normal(75, (N,))), g_mean=torch.tensor(rng.normal(76, (N, DY))))


@pytest.mark.parametrize("dtype", DTYPES, ids=["long_double", "float64"])
def test_svgp_rows_against_the_oracles_marginals_and_autograd(svgp, dtype):
    q, o = svgp, svgp["o"]
    n = lambda t: t.detach().numpy().copy()
    alpha, T, w, kd = n(q["alpha"]), n(q["alpha"] @ q["Q"]), n(q["w"]), n(q["kd"])
    got = rr.svgp_marginals(alpha, T, w, kd, dtype)
    mean, var = o.marginals(o.X)
    assert got["f_var"].dtype == dtype
    assert xr.rel_err(got["f_mean"], mean) < TOL and xr.rel_err(got["f_var"], var) < TOL
    # S = sum(g_var f_var) + sum(g_mean f_mean) as a function of (alpha, Q, w): autograd gives G_alpha, alpha^T diag(g_var) alpha
    # and alpha^T g_mean -- the products the two transposed operands exist for
    a_, Q_, w_ = [t.clone().requires_grad_(True) for t in (q["alpha"], q["Q"], q["w"])]
    S = (q["g_var"] * (q["kd"] + (a_ * (a_ @ Q_)).sum(1))).sum() + (q["g_mean"] * (a_ @ w_)).sum()
    S_o = (q["g_var"] * var).sum() + (q["g_mean"] * mean).sum()
    assert xr.rel_err(S.item(), S_o.item()) < TOL
    dalpha, dQ, dw = torch.autograd.grad(S, [a_, Q_, w_])
    bwd = rr.svgp_backward_rows(alpha, T, w, n(q["g_var"]), n(q["g_mean"]), dtype)
    assert xr.rel_err(bwd["T"], dalpha) < TOL
    assert np.array_equal(bwd["alphaT"], alpha.T.astype(dtype))
    assert xr.rel_err(bwd["galphaT"] @ bwd["alphaT"].T, dQ) < TOL and xr.rel_err(bwd["alphaT"] @ n(q["g_mean"]).astype(dtype), dw) < TOL
    # ... and through the oracle itself: dS/dq_mu = L^-T (alpha^T g_mean)
    (dmu,) = torch.autograd.grad(S_o, [o.raw["q_mu"]])
    want = torch.linalg.solve_triangular(q["L"].t(), dw, upper=True)
    assert xr.rel_err(dmu, want) < TOL
    assert xr.rel_err(np.linalg.solve(n(q["L"]).T, np.asarray(bwd["alphaT"] @ n(q["g_mean"]).astype(dtype), dtype=np.float64)), dmu) < TOL


def test_generator_properties():
    """what tests/test_gpu_rowkernels.py relies on: |a_i|^2 < 1, lambda well away from 0, cancellation rows that cancel exactly in
    either precision, and an fp64-vs-long-double error of every output that leaves room under the 1e-13 floor's rule."""
    for rows, m, dy in [(1, 1, 1), (2, 3, 2), (17, 65, 5), (35, 1026, 65), (19, 4225, 8)]:
        d = rr.inputs(rows, m, dy)
        assert np.all(np.sum(d["alpha"] ** 2, 1) < 1.0) and np.all(d["lam"] > 0.5) and np.all((d["kdiag"] >= 1.5) & (d["kdiag"] <= 2.5))
        assert len(d["cancel"]) == min(2, rows - 1) and d["Tf"].shape == (rows, rr.round_up(m, 16) + dy)
        for kd in (d["kdiag_fwd"], d["kdiag_shared"]):
            for dtype in DTYPES:
                lam = rr.fitc_forward_rows(d["At_fwd"], d["err"], kd, d["noise"], dtype)["lam"]
                assert all(lam[i] == dtype(d["noise"]) for i in d["cancel"]) and np.all(lam >= d["noise"])
        pairs = [(rr.svgp_marginals, (d["alpha"], d["T"], d["w"], d["kdiag"])),
                 (rr.svgp_backward_rows, (d["alpha"], d["T"], d["w"], d["g_var"], d["g_mean"])),
                 (rr.fitc_forward_rows, (d["At_fwd"], d["err"], d["kdiag_fwd"], d["noise"])),
                 (rr.fitc_backward_rows, (d["alpha"], d["Tf"], m, d["beta"], d["err"], d["lam"]))]
        for fn, args in pairs:
            hi, lo = fn(*args, dtype=rr.LD), fn(*args, dtype=np.float64)
            for k in hi:
                assert xr.rel_err(lo[k], hi[k]) < 1e-14, (fn.__name__, k, rows, m, dy)
