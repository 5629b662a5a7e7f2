"""
TEST INFRASTRUCTURE ONLY (never imported by the package) -- a host statement of expectation propagation for GP classification
(Rasmussen & Williams ch. 3.6 and 5.5.2) with a DENSE K, that shares nothing with the matrix-free native path of
gptorch_amd/models/ep.py.  The reference has no such model, so nothing here restates reference code.

Two arithmetics, as tests/_laplace_oracle.py (whose kernels, Cholesky, solves, case inputs and predict_f are reused):
  - dtype = np.float64: numpy / LAPACK / scipy.special, the pointwise terms in the closed forms the package uses (sites64);
  - dtype = np.longdouble: tests/_xref's Cholesky and solves; the pointwise terms from their DEFINITIONS in mpmath at 30 digits
    (sites_mp: plain phi / Phi, no tail tricks; the logit moments by the same H-node Gauss-Hermite rule with nodes and weights
    found in mpmath), rounded to long double.

    parallel sweep:  s = sqrt(max(tau, tiny)),  w = nu - tau m,  B = I + s K s = L L^T,  a = w - s B^-1 (s K w),  mu = m + K a,
                     sigma2_i = (1 / s_i) sum_j K_ij s_j Binv_ji,  cavity tau_c = 1 / sigma2 - tau, nu_c = mu / sigma2 - nu,
                     tilted moments, tau <- max(tau + rho (1 / s2_hat - tau_c - tau), 0),  nu <- nu + rho (mu_hat / s2_hat - nu_c - nu)
    stop:  change = max |undamped delta| <= tol (1 + max(|tau|, |nu|));  a stall: change <= 1e-6 of that scale and below neither of
           the two sweeps before  (until_stall: go on until the change stops shrinking in that sense);  then the factor AT the sites
    log Z_EP = sum e_i + 1/2 w^T K a - sum log L_ii,
           e_i = log Z^ + 1/2 log1p(tau / tau_c) + 1/2 (tau_c c (tau c - 2 w) - w^2) / (tau_c + tau),  c = nu_c / tau_c - m
    G = 1/2 a a^T - 1/2 R (R = s B^-1 s),  dlog Z_EP/dtheta = sum G dK/dtheta,  dlog Z_EP/dm = sum a

sequential(): R&W Algorithm 3.5 (one site at a time, rank-one updates of Sigma), for a host test of the fixed point.
"""
import math

import numpy as np
import scipy.special

from tests import _laplace_oracle as lo
from tests import _xref as xr

LD = xr.LD
TINY = np.finfo(np.float64).tiny
STALL_BELOW = 1e-6
MILLS_TERMS, MILLS_FROM = 200, -1.5
SITE_KEYS = ("tau_new", "nu_new", "lz", "mu_hat", "s2_hat", "site", "dtau", "dnu")
_RULES = {}


def rule64(H):
    return np.polynomial.hermite.hermgauss(int(H))


def rule_mp(H, dps=40):
    """the physicists' Gauss-Hermite nodes and weights in mpmath: Newton's iteration on H_H from numpy's nodes,
    w = 2^(H-1) H! sqrt(pi) / (H H_(H-1)(x))^2."""
    import mpmath as mp
    if (H, dps) not in _RULES:
        with mp.workdps(dps):
            xs, ws = [], []
            for x0 in np.polynomial.hermite.hermgauss(int(H))[0]:
                x = mp.mpf(float(x0))
                for _ in range(6):
                    x = x - mp.hermite(H, x) / (2 * H * mp.hermite(H - 1, x))
                xs.append(x)
                ws.append(mp.mpf(2) ** (H - 1) * mp.factorial(H) * mp.sqrt(mp.pi) / (H * mp.hermite(H - 1, x)) ** 2)
            _RULES[(H, dps)] = (xs, ws)
    return _RULES[(H, dps)]


# ---- the per-point half of a sweep: what gpn_ep_sites computes ------------------------------------------------------------------------
LOGIT_VARIANTS = 6


def sites64(lik, y, m, mu, sigma2, tau, nu, damping, H=20, variant=0):
    """plain fp64, the closed forms of csrc/lik_point.h -> dict of SITE_KEYS arrays (tau_new / nu_new: the damped update).
    variant (logit; < LOGIT_VARIANTS): the same sums over the nodes in another order and with the node's argument associated the
    other way -- equally valid fp64 evaluations whose spread shows the rounding error of a sum that cancels (variant 0: numpy's
    pairwise sum over the nodes as stored)."""
    y, m, mu, sigma2, tau, nu = (np.asarray(v, dtype=np.float64) for v in (y, m, mu, sigma2, tau, nu))
    t = 2.0 * y - 1.0
    prec = 1.0 / sigma2
    tau_c, nu_c = prec - tau, mu * prec - nu
    v_c = 1.0 / tau_c
    mu_c = nu_c * v_c
    if lik == "probit":
        d = 1.0 + v_c
        rs = 1.0 / np.sqrt(d)
        z = t * mu_c * rs
        zn, zp = np.minimum(z, 0.0), np.maximum(z, 0.0)
        neg = math.sqrt(2.0 / math.pi) / scipy.special.erfcx(-zn * math.sqrt(0.5))
        pos = np.exp(-0.5 * zp * zp) / math.sqrt(2.0 * math.pi) / (1.0 - 0.5 * scipy.special.erfc(zp * math.sqrt(0.5)))
        r = np.where(z < 0.0, neg, pos)
        x = np.maximum(-z, -MILLS_FROM)
        e = np.zeros_like(x)
        for k in range(MILLS_TERMS, 1, -1):
            e = k / (x + e)
        D = 1.0 / (x + e)
        tail = z < MILLS_FROM
        r = np.where(tail, x + D, r)
        w = np.where(tail, r * D, r * (z + r))
        omw = np.where(tail, D * (e - D), 1.0 - w)
        h = np.where(tail, e * D, 1.0 + z * (z + r))
        q = 1.0 + v_c * omw
        lz = scipy.special.log_ndtr(z)
        mu_hat = np.where(tail, t * (D * v_c - x) * rs, mu_c + v_c * (t * r * rs))
        s2_hat = v_c * q / d
        tau_full = w / q
        nu_full = t * r * h / (rs * q)
    elif lik == "logit":
        xs, ws = rule64(H)
        sd = np.sqrt(v_c)
        step = sd * math.sqrt(2.0)

        def logsig(f):
            return np.minimum(f, 0.0) - np.log1p(np.exp(-np.abs(f)))

        order = (np.arange(H), np.arange(H)[::-1], np.concatenate([np.arange(0, H, 2), np.arange(1, H, 2)]))[variant % 3]

        def total(a):
            return a.sum(1) if variant == 0 else np.cumsum(a[:, order], 1)[:, -1]

        lmax = logsig(t * mu_c + step * np.max(np.abs(xs)))
        arg = t[:, None] * (mu_c[:, None] + step[:, None] * xs[None, :]) if variant < 3 else \
            (t * mu_c)[:, None] + (t * step)[:, None] * xs[None, :]
        gk = ws[None, :] * np.exp(logsig(arg) - lmax[:, None])
        s0 = total(gk)
        m1 = math.sqrt(2.0) * (total(gk * xs[None, :]) / s0)
        c = math.sqrt(2.0) * xs[None, :] - m1[:, None]
        s2, sm = total(gk * (c * c)), total(gk * (1.0 - c * c))
        lz = lmax + np.log(s0 / math.sqrt(math.pi))
        mu_hat = mu_c + sd * m1
        s2_hat = v_c * (s2 / s0)
        tau_full = (sm / s2) / v_c
        nu_full = mu_hat * tau_full + m1 / sd
    else:
        raise ValueError(lik)
    c, w = mu_c - m, nu - tau * m
    site = lz + 0.5 * np.log1p(tau * v_c) + 0.5 * (tau_c * c * (tau * c - 2.0 * w) - w * w) / (tau_c + tau)
    dtau, dnu = tau_full - tau, nu_full - nu
    return {"tau_new": np.maximum(tau + damping * dtau, 0.0), "nu_new": nu + damping * dnu, "lz": lz, "mu_hat": mu_hat, "s2_hat": s2_hat,
            "site": site, "dtau": dtau, "dnu": dnu}


def sites_mp(lik, y, m, mu, sigma2, tau, nu, damping, H=20, dps=40):
    """the definitions themselves in mpmath -> dict of SITE_KEYS lists of mpf.  Inputs may be long double (both halves are kept)."""
    import mpmath as mp

    def up(v):
        hi = float(v)
        return mp.mpf(hi) + mp.mpf(float(LD(v) - LD(hi)))

    out = {k: [] for k in SITE_KEYS}
    with mp.workdps(dps):
        rho = up(damping)
        if lik == "logit":
            xs, ws = rule_mp(H, dps)
        for yi, mi, mui, s2i, taui, nui in zip(*(np.asarray(v).ravel() for v in (y, m, mu, sigma2, tau, nu))):
            t, mi, mui, s2i, taui, nui = 2 * up(yi) - 1, up(mi), up(mui), up(s2i), up(taui), up(nui)
            tau_c, nu_c = 1 / s2i - taui, mui / s2i - nui
            v_c = 1 / tau_c
            mu_c = nu_c * v_c
            if lik == "probit":
                z = t * mu_c / mp.sqrt(1 + v_c)
                Phi = mp.erfc(-z / mp.sqrt(2)) / 2
                r = mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi) / Phi
                lz = mp.log(Phi)
                mu_hat = mu_c + t * v_c * r / mp.sqrt(1 + v_c)
                s2_hat = v_c - v_c * v_c * r * (z + r) / (1 + v_c)
            else:
                fs = [mu_c + mp.sqrt(2 * v_c) * x for x in xs]
                gs = [w / (1 + mp.exp(-t * f)) for w, f in zip(ws, fs)]
                Z = mp.fsum(gs)
                lz = mp.log(Z / mp.sqrt(mp.pi))
                mu_hat = mp.fsum(g * f for g, f in zip(gs, fs)) / Z
                s2_hat = mp.fsum(g * (f - mu_hat) ** 2 for g, f in zip(gs, fs)) / Z
            dtau, dnu = 1 / s2_hat - tau_c - taui, mu_hat / s2_hat - nu_c - nui
            c, w = mu_c - mi, nui - taui * mi
            site = lz + mp.log1p(taui * v_c) / 2 + (tau_c * c * (taui * c - 2 * w) - w * w) / (tau_c + taui) / 2
            for k, v in zip(SITE_KEYS, (max(taui + rho * dtau, mp.mpf(0)), nui + rho * dnu, lz, mu_hat, s2_hat, site, dtau, dnu)):
                out[k].append(v)
    return out


def sites_ld(lik, y, m, mu, sigma2, tau, nu, damping, H=20):
    return {k: np.array([lo._mp_to_ld(x) for x in v], dtype=LD) for k, v in sites_mp(lik, y, m, mu, sigma2, tau, nu, damping, H, dps=30).items()}


class EPOracle(lo.LaplaceOracle):
    """lik: "probit" | "logit"; the rest as LaplaceOracle.  search() -> self with tau, nu, a, Ka, s, L, mu, sigma2, mu_hat, s2_hat,
    sweeps, stalled; gradients w.r.t. log variance, log length_scales [d or 1] and the mean."""

    def __init__(self, x, y, kind, lik, variance, length_scales, ARD=False, mean=None, dtype=np.float64, H=20):
        if lik not in ("probit", "logit"):
            raise ValueError(lik)
        super().__init__(x, y, kind, lik, variance, length_scales, ARD=ARD, mean=mean, dtype=dtype)
        self.H = int(H)
        self.mvec = np.full(self.n, self.m, dtype=self.dt)

    def sites(self, mu, sigma2, tau, nu, damping):
        return (sites_ld if self.dt is LD else sites64)(self.lik, self.y, self.mvec, mu, sigma2, tau, nu, damping, self.H)

    def posterior(self, tau, nu):
        """steps 1-3 of a sweep -> (s, L, a, K a, mu, sigma2)"""
        dt, K = self.dt, self.Kf
        s = np.sqrt(np.maximum(tau, dt(TINY)))
        w = nu - tau * self.mvec
        L = self._chol(np.eye(self.n, dtype=dt) + s[:, None] * K * s[None, :])
        a = w - s * self._ltsolve(L, self._lsolve(L, s * (K @ w)))
        Ka = K @ a
        Li = self._lsolve(L, np.eye(self.n, dtype=dt))
        sigma2 = np.sum(K * (Li.T @ Li) * s[None, :], 1) / s
        return s, L, a, Ka, self.mvec + Ka, sigma2

    def search(self, sites0=None, tol=1e-10, max_sweeps=200, damping=0.8, until_stall=False):
        dt = self.dt
        tau = np.zeros(self.n, dtype=dt) if sites0 is None else np.asarray(sites0[0], dtype=dt).copy()
        nu = np.zeros(self.n, dtype=dt) if sites0 is None else np.asarray(sites0[1], dtype=dt).copy()
        sweeps, stalled, before = 0, False, []
        while True:
            if sweeps >= max_sweeps:
                raise RuntimeError("no convergence in %d sweeps" % max_sweeps)
            _, _, _, _, mu, sigma2 = self.posterior(tau, nu)
            up = self.sites(mu, sigma2, tau, nu, dt(damping))
            tau, nu = up["tau_new"], up["nu_new"]
            sweeps += 1
            change = max(np.max(np.abs(up["dtau"])), np.max(np.abs(up["dnu"])))
            scale = 1 + max(np.max(np.abs(tau)), np.max(np.abs(nu)))
            if until_stall:
                if change == 0 or (len(before) == 2 and change <= tol * scale and change >= max(before)):
                    break
            else:
                if change <= tol * scale:
                    break
                if len(before) == 2 and change <= STALL_BELOW * scale and change >= max(before):
                    stalled = True
                    break
            before = (before + [change])[-2:]
        self.sweeps, self.stalled = sweeps, stalled
        return self.settle(tau, nu)

    def settle(self, tau, nu):
        """the state at given sites: the factor AT the sites, the posterior, the cavity and the moments, no update."""
        self.tau, self.nu = np.asarray(tau, dtype=self.dt), np.asarray(nu, dtype=self.dt)
        self.s, self.L, self.a, self.Ka, self.mu, self.sigma2 = self.posterior(self.tau, self.nu)
        self.final = self.sites(self.mu, self.sigma2, self.tau, self.nu, self.dt(1.0))
        self.mu_hat, self.s2_hat = self.final["mu_hat"], self.final["s2_hat"]
        return self

    def log_evidence(self):
        w = self.nu - self.tau * self.mvec
        return np.sum(self.final["site"]) + self.dt(0.5) * (w @ self.Ka) - np.sum(np.log(np.diag(self.L)))

    def log_evidence_direct(self):
        """sum log Z~_i + log N(mu~ | m, K + Sigma~) as written (R&W eqs. 3.65 and 3.66); divides by tau."""
        dt = self.dt
        tau_c = 1 / self.sigma2 - self.tau
        mu_c = (self.mu / self.sigma2 - self.nu) / tau_c
        v_c, v_s, mu_s = 1 / tau_c, 1 / self.tau, self.nu / self.tau
        log_zt = self.final["lz"] + dt(0.5) * np.log(2 * dt(np.pi)) + dt(0.5) * np.log(v_c + v_s) + (mu_c - mu_s) ** 2 / (2 * (v_c + v_s))
        C = self._chol(self.Kf + np.diag(v_s))
        h = self._lsolve(C, mu_s - self.mvec)
        return np.sum(log_zt) - dt(0.5) * (h @ h) - np.sum(np.log(np.diag(C))) - dt(0.5) * self.n * np.log(2 * dt(np.pi))

    def loss_grads(self):
        dt, K, s = self.dt, self.Kf, self.s
        Li = self._lsolve(self.L, np.eye(self.n, dtype=dt))
        G = dt(0.5) * (np.outer(self.a, self.a) - s[:, None] * (Li.T @ Li) * s[None, :])
        g_ls = np.empty(self.d, dtype=dt)
        GB = G * self.Bf
        for c in range(self.d):
            t = (self.X[:, c:c + 1] - self.X[None, :, c]) / self.ls[c]
            g_ls[c] = np.sum(GB * t * t)
        return [-np.array([np.sum(G * K)]), -(g_ls if self.ARD else np.array([g_ls.sum()])), -np.array([np.sum(self.a)])]

    def sequential(self, tol=1e-13, max_sweeps=200):
        """R&W Algorithm 3.5 (fp64): sites visited one at a time, Sigma by rank-one updates, recomputed from the factor after
        every sweep -> (tau, nu, mu, sigma2) at its fixed point."""
        K, m = self.Kf, self.mvec
        tau, nu = np.zeros(self.n), np.zeros(self.n)
        Sigma, mu = K.copy(), m.copy()
        for _ in range(max_sweeps):
            change = 0.0
            for i in range(self.n):
                up = sites64(self.lik, self.y[i:i + 1], m[i:i + 1], mu[i:i + 1], Sigma[i:i + 1, i], tau[i:i + 1], nu[i:i + 1], 1.0, self.H)
                dtau = float(up["tau_new"][0] - tau[i])
                change = max(change, abs(dtau), abs(float(up["nu_new"][0] - nu[i])))
                tau[i], nu[i] = up["tau_new"][0], up["nu_new"][0]
                si = Sigma[:, i].copy()
                Sigma -= (dtau / (1.0 + dtau * si[i])) * np.outer(si, si)
                mu = m + Sigma @ (nu - tau * m)
            s, L, a, Ka, mu, sigma2 = self.posterior(tau, nu)
            V = self._lsolve(L, s[:, None] * K)
            Sigma = K - V.T @ V
            if change <= tol * (1.0 + max(np.max(np.abs(tau)), np.max(np.abs(nu)))):
                return tau, nu, mu, sigma2
        raise RuntimeError("sequential EP: no convergence in %d sweeps" % max_sweeps)


def build_oracle(case, inp, dtype=np.float64):
    return EPOracle(inp["x"], inp["y"], case["kind"], case["lik"], case["variance"], case["length_scales"], ARD=bool(case["ARD"]),
                    mean=case["mean"], dtype=dtype, H=int(case.get("H", 20)))


def build_model(case, inp):
    import torch
    from gptorch_amd import kernels, likelihoods, mean_functions
    from gptorch_amd.models import EPGP
    d = int(case["d"])
    ls = np.asarray(case["length_scales"], dtype=np.float64) if case["ARD"] else float(np.atleast_1d(case["length_scales"])[0])
    k = getattr(kernels, case["kind"])(d, variance=float(case["variance"]), length_scales=ls, ARD=bool(case["ARD"]))
    lik = likelihoods.Bernoulli(case["lik"])
    lik.num_gauss_hermite_points = int(case.get("H", 20))
    mean = None if case["mean"] is None else mean_functions.Constant(1, torch.tensor([float(case["mean"])], dtype=torch.float64))
    return EPGP(inp["x"], inp["y"], k, lik, mean_function=mean)
