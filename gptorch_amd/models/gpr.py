"""
Exact GP regression (gptorch/models/gpr.py) over the native pipeline.

log_likelihood:  one autograd node = fused K(X)+sigma_n^2 I assembly into the
factor buffer -> blocked MFMA Cholesky with the residual (y - m)^T riding along
as extra rows (forward substitution for free) -> log-det / ||alpha||^2
reduction.  _predict re-uses the cached factor when neither the parameters nor
the inputs changed (the reference re-factorises on every call, gpr.py:104).
"""
import torch

from .. import _ops, kernels
from .base import GPModel


INVERSE_AFTER_CALLS = 3      # predictions with one cached factor before L^-1 is formed (see _predict); N < 4096 only
BLOCKED_AFTER_CALLS = 1      # ... and before the 1024 x 1024 diagonal blocks are inverted (N >= 4096)


class GPR(GPModel):
    def __init__(self, x, y, kernel, mean_function=None, likelihood=None, name="gpr", objective="lml", folds=None):
        """objective: what loss() / optimize() fit -- "lml", the log marginal likelihood (the reference's only objective), "loo",
        the leave-one-out log predictive density (loo_log_predictive), or "kfold", the k-fold log predictive density in closed form
        (kfold_log_predictive).  log_likelihood() is the LML in every case.
        folds (objective="kfold" only; required there): an int k >= 2 -- np.array_split(np.arange(n), k): CONTIGUOUS blocks in data
        order, no shuffling (shuffle the data, or pass index arrays, when the order carries structure) -- or a sequence of integer
        index arrays that partition range(n): every index exactly once, no empty fold, at least two folds (ValueError otherwise).
        Folds are padded to the largest: a partition with k * round_up(m_max, 16) > 4 round_up(n, 16) raises NotImplementedError (all-singleton
        folds among them: that is objective="loo")."""
        super().__init__(x, y, kernel, likelihood, mean_function, name)
        if objective not in ("lml", "loo", "kfold"):
            raise ValueError("objective must be 'lml', 'loo' or 'kfold'; got %r" % (objective,))
        self.objective = objective
        self.folds = None
        if objective == "kfold":
            self.folds = _ops.FoldTable(folds, self.X.shape[0])
        elif folds is not None:
            raise ValueError("folds belongs to objective='kfold'; got objective=%r" % (objective,))
        self._holder = {}        # reusable factor buffer for the training loop
        self._predict_cache = None
        self._predict_calls = 0

    def _stationary(self):
        """the kernel if it is one of the native stationary kinds (fused assembly -> factor
        path), else None (composite / linear / static kernels: dense-K path)."""
        k = self.kernel
        return k if isinstance(k, kernels.Stationary) and k._kind is not None else None

    def _expression(self, x):
        """the fused-expression program of a composite kernel (gptorch_amd._expr) or None (dense-K path)."""
        k = self.kernel
        if not isinstance(k, kernels.Combination) or not x.is_cuda or x.requires_grad:
            return None
        prog = k.fused_program()
        return prog if prog is not None and prog.grad_supported(x.shape[1]) else None

    def log_likelihood(self, x=None, y=None):
        """gpr.py:47-67; returns a tensor of shape (1,)."""
        x = x if x is not None else self.X
        y = y if y is not None else self.Y
        if not x.shape[0] == y.shape[0]:
            raise ValueError("X and Y must have same # data.")
        k = self._stationary()
        resid = y - self.mean_function(x)
        if k is None:
            prog = self._expression(x)
            if prog is not None:
                # composite kernel with native leaves (e.g. the reference's example Linear + Rbf + Constant,
                # examples/regression_1d.py:34-53): fused assembly into the factor buffer, expression sweeps in the backward
                from .. import _expr
                return _expr.ExprLogLik.apply(x, resid, self.likelihood.variance.transform(), prog, self._holder, *prog.params())
            return _ops.DenseLogLik.apply(self.kernel.K(x), resid, self.likelihood.variance.transform())
        return _ops.GPRLogLik.apply(x, resid, k.variance.transform(), k.length_scales.transform(),
                                    self.likelihood.variance.transform(), k._kind, self._holder)

    def loo_log_predictive(self, x=None, y=None):
        """sum_i log p(y_i | X, y_-i, theta), the leave-one-out log predictive density in closed form from ONE factorisation
        (Rasmussen & Williams 5.4.2, eqs. 5.10-5.13); differentiable, shape (1,).  Kernels without a native kind (composites
        included) hand their dense K(x) to the same native steps."""
        x = x if x is not None else self.X
        y = y if y is not None else self.Y
        if not x.shape[0] == y.shape[0]:
            raise ValueError("X and Y must have same # data.")
        k = self._stationary()
        resid = y - self.mean_function(x)
        if k is None:
            return _ops.DenseLooLik.apply(self.kernel.K(x), resid, self.likelihood.variance.transform())
        return _ops.GPRLooLik.apply(x, resid, k.variance.transform(), k.length_scales.transform(),
                                    self.likelihood.variance.transform(), k._kind, self._holder)

    def loo_predict(self, x=None, y=None):
        """(mean [n, dy], var [n, dy]) of every OBSERVATION y_i given all the others (noise included: the predictive that
        loo_log_predictive scores), from one factorisation; no gradients."""
        self._auto_place()
        x = x if x is not None else self.X
        y = y if y is not None else self.Y
        if not x.shape[0] == y.shape[0]:
            raise ValueError("X and Y must have same # data.")
        with torch.no_grad():
            k = self._stationary()
            resid = y - self.mean_function(x)
            noise = self.likelihood.variance.transform()
            if k is None:
                f = _ops.cholesky_factor(self._compute_kyy(x), rhs=resid)
            else:
                f = _ops.kernel_factor(k._kind, x, k.variance.transform(), k.length_scales.transform(), noise, R=resid)
            s = _ops.LooState(f, want_w=False)
            return y - s.qt.t(), s.var[:, None].expand(y.shape[0], y.shape[1]).clone()

    def _fold_table(self, n, folds):
        if folds is None:
            folds = self.folds
        if not isinstance(folds, _ops.FoldTable):
            folds = _ops.FoldTable(folds, n)
        if folds.n != n:
            raise ValueError("folds partition range(%d) but the data have %d rows" % (folds.n, n))
        return folds

    def kfold_log_predictive(self, x=None, y=None, folds=None):
        """sum_f log p(y_I | X, y_-I, theta) over the folds (default: the constructor's), the k-fold log predictive density in closed
        form from ONE factorisation and the diagonal blocks of Kyy^-1; differentiable w.r.t. kernel parameters, noise and mean
        function, shape (1,).  Kernels without a native kind (composites included) hand their dense K(x) to the same native steps."""
        x = x if x is not None else self.X
        y = y if y is not None else self.Y
        if not x.shape[0] == y.shape[0]:
            raise ValueError("X and Y must have same # data.")
        table = self._fold_table(x.shape[0], folds)
        k = self._stationary()
        resid = y - self.mean_function(x)
        if k is None:
            return _ops.DenseKFoldLik.apply(self.kernel.K(x), resid, self.likelihood.variance.transform(), table)
        return _ops.GPRKFoldLik.apply(x, resid, k.variance.transform(), k.length_scales.transform(),
                                      self.likelihood.variance.transform(), k._kind, self._holder, table)

    def kfold_predict(self, x=None, y=None, folds=None):
        """(mean [n, dy], var [n, dy]) in DATA order: for each point the marginal predictive of the OBSERVATION (noise included) from
        the model that never saw the point's fold -- what kfold_log_predictive scores, without the covariances inside a fold; from
        one factorisation; no gradients."""
        self._auto_place()
        x = x if x is not None else self.X
        y = y if y is not None else self.Y
        if not x.shape[0] == y.shape[0]:
            raise ValueError("X and Y must have same # data.")
        table = self._fold_table(x.shape[0], folds)
        with torch.no_grad():
            k = self._stationary()
            resid = y - self.mean_function(x)
            noise = self.likelihood.variance.transform()
            if k is None:
                f = _ops.cholesky_factor(self._compute_kyy(x), rhs=resid)
            else:
                f = _ops.kernel_factor(k._kind, x, k.variance.transform(), k.length_scales.transform(), noise, R=resid)
            s = _ops.KFoldState(f, table, want_w=False)
            return y - s.qt.t(), s.var[:, None].expand(y.shape[0], y.shape[1]).clone()

    def _loss(self, *args, **kwargs):
        if self.objective == "lml":
            return super()._loss(*args, **kwargs)
        self._auto_place()
        if self.objective == "kfold":
            return -(self.kfold_log_predictive(*args, **kwargs) + self.log_prior())
        return -(self.loo_log_predictive(*args, **kwargs) + self.log_prior())

    def _compute_kyy(self, x=None):
        """K(x) + sigma_n^2 I as a dense tensor (gpr.py:69-86); API parity only --
        the training / predict paths never materialise it outside the factor buffer."""
        x = x if x is not None else self.X
        k = self._stationary()
        if k is None:
            Kyy = self.kernel.K(x).clone()
            Kyy.diagonal().add_(self.likelihood.variance.transform()[0])
            return Kyy
        return _ops.kernel_matrix(k._kind, x, None, k.variance.transform(), k.length_scales.transform(),
                                  noise=self.likelihood.variance.transform())

    def _factor_for_predict(self, x):
        """the factor of Kyy with L^-1 (y - m) riding along, kept between predictions (GPModel._cached_state)"""
        k = self._stationary()
        with torch.no_grad():
            var, ls, noise = k.variance.transform(), k.length_scales.transform(), self.likelihood.variance.transform()
            f = self._cached_state(k._kind, x, lambda: _ops.kernel_factor(k._kind, x, var, ls, noise, R=self.Y - self.mean_function(x)))
            self._predict_calls += 1
        return f, var, ls

    def _predict_dense(self, x_new, diag, x):
        """gpr.py:88-117 for a kernel without a native kind: the kernel's own K() calls, the
        native factorisation / right-solves / contractions."""
        with torch.no_grad():
            n, ns = x.shape[0], x_new.shape[0]
            # the factor is kept between predictions exactly as for the native kinds (_factor_for_predict)
            f = self._cached_state("dense", x, lambda: _ops.cholesky_factor(self._compute_kyy(x), rhs=self.Y - self.mean_function(x)))
            self._predict_calls += 1
            Bt = _ops.padded_like_factor(f, ns)
            Bt[:ns, :n] = self.kernel.K(x_new, x)
            f.solve_right_lt(Bt, ns)                                        # A^T = K(x*, x) L^-T
            mean = _ops.gemm_nt(Bt, f.A[n:], ns, f.e, _ops.round_up(n, 16)) + self.mean_function(x_new)
            if diag:
                v = self.kernel.Kdiag(x_new) - _ops.row_sumsq(Bt, ns, n)
                return mean, v[:, None].expand_as(mean)
            cov = self.kernel.K(x_new).clone()
            _ops.gemm_nt(Bt, Bt, ns, ns, _ops.round_up(n, 16), alpha=-1.0, beta=1.0, C=cov)
            return mean, cov

    def _predict(self, x_new, diag=True, x=None):
        """p(F* | Y) (gpr.py:88-117): mean [n*, dy]; var [n*, dy] (diag) or cov [n*, n*]."""
        x = x if x is not None else self.X
        k = self._stationary()
        if k is None:
            return self._predict_dense(x_new, diag, x)
        f, var, ls = self._factor_for_predict(x)
        with torch.no_grad():
            # The first prediction with a factor walks the right-solve recursion down to the 128-wide leaf inverses (~2 n / 128
            # small launches).  From the second on (N >= 4096): the inverses of the 1024 x 1024 diagonal blocks are formed once
            # (n 1024^2 / 3 flops) and the solve is n / 1024 steps of two large contractions (2.3 -> 1.3 ms at N = 8192, 1024
            # test points).  Below 4096 rows: from the third prediction on, one contraction with the explicit inverse.
            big = x.shape[0] >= _ops.BLOCKED_PREDICT_MIN_N
            mean_f, v = _ops.gpr_predict(k._kind, x, x_new, var, ls, f, diag=diag,
                                         use_inverse=(not big) and self._predict_calls >= INVERSE_AFTER_CALLS,
                                         mean_new=self.mean_function(x_new), blocked=big and self._predict_calls > BLOCKED_AFTER_CALLS)
            var_f = v[:, None].expand_as(mean_f) if diag else v
        return mean_f, var_f


def __getattr__(name):
    """The lock-step entry points, their grouping helpers and multi_start_optimize lived in this module and are still read from
    it (bench.py: two_lane_streams): such a name resolves to its present home, always with that module's current value.
    Assigning one here does NOT reach the code that uses it: patch models/_lockstep.py or models/_multistart.py."""
    from . import _lockstep, _multistart
    for home in (_lockstep, _multistart):
        if name in vars(home) and not name.startswith("__"):
            return getattr(home, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
