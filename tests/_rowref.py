"""
TEST INFRASTRUCTURE ONLY (never imported by the package) -- what include/gpnative.h promises for the four row kernels of the sparse
models (gpn_svgp_marginals, gpn_svgp_backward_rows, gpn_fitc_forward_rows, gpn_fitc_backward_rows; csrc/svgp.hip, csrc/fitc.hip,
csrc/rowkernels.h), as plain numpy statements on the LOGICAL arrays: no leading dimensions, no padding, no tiles.

Every function takes the fp64 arrays handed to the kernel and a `dtype`: numpy's long double (the reference) or float64 (the plain
fp64 evaluation of the same statement -- its distance from the long-double one is the e64 that tests/_xref.tol's rule turns into
a tolerance; it is never measured against the code under test).

`inputs(rows, m, dy)` draws the arrays of a case: alpha uniform in [-1, 1] / sqrt(m) (so |a_i|^2 < 1), kdiag in [1.5, 2.5], noise
0.05, everything else standard normal -- lambda = kdiag - |a_i|^2 + noise stays above 0.5 --, and for the FITC forward up to two
CANCELLATION rows: a single entry 1.5 against kdiag = 2.25, so that lambda is exactly `noise` (what FITC sees where Z holds a row
of X).
"""
import numpy as np

LD = np.longdouble
NOISE = 0.05
KDIAG_SHARED = 2.25                # kdiag_stride 0: the one value of every row (the cancellation rows need 1.5^2)


def round_up(a, b):
    return (a + b - 1) // b * b


def _c(a, dtype):
    return np.asarray(a, dtype=dtype)


def svgp_marginals(alpha, T, w, kdiag, dtype=LD):
    """f_var[i] = kdiag[i] + sum_j alpha_ij T_ij,  f_mean = alpha w  -> dict(f_mean [rows, dy], f_var [rows])."""
    a, t, w, kd = _c(alpha, dtype), _c(T, dtype), _c(w, dtype), _c(kdiag, dtype)
    return dict(f_mean=a @ w, f_var=kd + np.sum(a * t, axis=1))


def svgp_backward_rows(alpha, T, w, g_var, g_mean, dtype=LD):
    """G_alpha = 2 g_var_i T_i + g_mean_i w^T and the two transposed operands -> dict(T [rows, m], alphaT, galphaT [m, rows])."""
    a, t, w, gv, gm = _c(alpha, dtype), _c(T, dtype), _c(w, dtype), _c(g_var, dtype), _c(g_mean, dtype)
    return dict(T=2 * gv[:, None] * t + gm @ w.T, alphaT=a.T.copy(), galphaT=(gv[:, None] * a).T.copy())


def fitc_forward_rows(At, err, kdiag, noise, dtype=LD):
    """lambda_i = kdiag_i - |At_i|^2 + noise; At_i / sqrt(lambda_i); (err_i / sqrt(lambda_i))^T; the two scalar sums
    -> dict(lam [rows], At [rows, m], errT [dy, rows], out2 [2])."""
    a, e, kd = _c(At, dtype), _c(err, dtype), _c(kdiag, dtype)
    lam = kd - np.sum(a * a, axis=1) + dtype(noise)
    s = np.sqrt(lam)
    return dict(lam=lam, At=a / s[:, None], errT=(e / s[:, None]).T.copy(),
                out2=np.array([np.sum(np.log(lam)), np.sum(e * e / lam[:, None])], dtype=dtype))


def fitc_backward_rows(alpha, T, m, beta, err, lam, dtype=LD):
    """T [rows, >= round_up(m, 16) + dy] is the kernel's whole input: alpha B^-1 in columns < m and the alpha beta block from
    column round_up(m, 16) on, which is READ here, not recomputed from alpha and beta.
    -> dict(r [rows, dy], g [rows], T [rows, m] (the rows of dF/dA^T), alphaT, galphaT [m, rows])."""
    a, t, b, e, lam = _c(alpha, dtype), _c(T, dtype), _c(beta, dtype), _c(err, dtype), _c(lam, dtype)
    dy, mp = e.shape[1], round_up(m, 16)
    tm, ab = t[:, :m], t[:, mp:mp + dy]
    r = (e - ab) / lam[:, None]
    h = np.sum(a * tm, axis=1)
    g = np.sum(r * r, axis=1) - dy * (1 / lam - h / (lam * lam))
    return dict(r=r, g=g, T=r @ b.T - (dy / lam)[:, None] * tm - g[:, None] * a, alphaT=a.T.copy(), galphaT=(g[:, None] * a).T.copy())


def inputs(rows, m, dy, seed=0):
    """the fp64 arrays of one (rows, m, dy) case, logical shapes.  Keys: alpha, T [rows, m]; w, beta [m, dy]; kdiag, g_var [rows];
    g_mean, err [rows, dy]; noise; lam [rows] (the forward's lambda of alpha, in fp64: the backward's input); Tf [rows,
    round_up(m, 16) + dy] (FITC's T, zeros between the two blocks: the layouts of the test overwrite them); At_fwd, kdiag_fwd
    (alpha / kdiag with the cancellation rows written in: rows 0 and rows - 1 when rows >= 3, row 0 when rows == 2, none for one
    row -- every case keeps an ordinary row); kdiag_shared: the kdiag_stride = 0 variant, one value for all rows, the cancellation
    rows' (they cancel under it as well)."""
    g = np.random.RandomState(1000003 * rows + 1009 * m + dy + seed)
    d = {}
    d["alpha"] = g.uniform(-1.0, 1.0, (rows, m)) / np.sqrt(m)
    d["T"] = g.standard_normal((rows, m))
    d["w"] = g.standard_normal((m, dy))
    d["beta"] = g.standard_normal((m, dy))
    d["kdiag"] = g.uniform(1.5, 2.5, rows)
    d["g_var"] = g.standard_normal(rows)
    d["g_mean"] = g.standard_normal((rows, dy))
    d["err"] = g.standard_normal((rows, dy))
    d["noise"] = NOISE
    d["lam"] = d["kdiag"] - np.sum(d["alpha"] ** 2, axis=1) + NOISE
    mp = round_up(m, 16)
    d["Tf"] = np.zeros((rows, mp + dy))
    d["Tf"][:, :m] = d["T"]
    d["Tf"][:, mp:] = g.standard_normal((rows, dy))
    cancel = [] if rows < 2 else [0] if rows == 2 else [0, rows - 1]
    d["cancel"] = cancel
    d["At_fwd"], d["kdiag_fwd"] = d["alpha"].copy(), d["kdiag"].copy()
    for i, col in zip(cancel, (m - 1, 0)):              # one at the last column (the odd tail when m is odd), one at the first
        d["At_fwd"][i] = 0.0
        d["At_fwd"][i, col] = 1.5
        d["kdiag_fwd"][i] = 2.25
    d["kdiag_shared"] = np.full(rows, KDIAG_SHARED)
    return d
