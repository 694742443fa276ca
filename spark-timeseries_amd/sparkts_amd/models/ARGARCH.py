"""MI355X-native ARGARCH (GARCH.scala:56-70, 198-260) over the HIP engine.

AR(1) with an intercept and GARCH(1,1) errors: y_t = c + phi * y_{t-1} + eta_t, h_t = omega + alpha * eta_{t-1}^2 +
beta * h_{t-1}. `fit_model` is ARGARCH.fitModel: Autoregression.fitModel(ts), then GARCH.fitModel on that model's
residuals -- with GARCH.fitModel's two reproduced properties (models/GARCH.py). On the device the two stages are fused:
the residuals are formed inside the GARCH passes and never stored. `sc` is accepted and ignored.
"""
import numpy as np

from .. import _lib
from .ARIMA import ARIMAFitError, SingularMatrixException  # noqa: F401  (what fit_model / model(i) raise)
from .GARCH import raise_for_status


class ARGARCHFitBatchResult:
    """Per-series outputs of a batched ARGARCH fit (the arrays arima_argarch_fit_batch fills)."""

    def __init__(self, r, device=None):
        self.coefficients = r["coef"]            # (N, 5): c, phi, omega, alpha, beta
        self.log_likelihood = r["ll"]            # GARCHModel.logLikelihood of the AR residuals
        self.status = r["status"]
        self.n_eval = r["n_eval"]
        self.n_grad = r["n_grad"]
        self._device = device

    c = property(lambda self: self.coefficients[:, 0])
    phi = property(lambda self: self.coefficients[:, 1])
    omega = property(lambda self: self.coefficients[:, 2])
    alpha = property(lambda self: self.coefficients[:, 3])
    beta = property(lambda self: self.coefficients[:, 4])

    def model(self, i):
        raise_for_status(self.status[i])
        return ARGARCHModel(*(float(v) for v in self.coefficients[i]), device=self._device)

    @property
    def converged(self):
        return self.status == _lib.ST_OK


def fit_models(series, device=None):
    """Batched ARGARCH.fitModel: `series` is (N, T) float64, one row per series. Never raises for per-series failures;
    inspect `.status` (a series that failed in either stage has five NaN parameters)."""
    return ARGARCHFitBatchResult(_lib.Engine.get(device).argarch_fit_batch(series), device)


def fit_model(ts, sc=None, device=None):
    """ARGARCH.fitModel (GARCH.scala:63-69), one series. Raises the reference's exception on failure."""
    ts = np.asarray(ts, dtype=np.float64).ravel()
    return fit_models(ts[None, :], device=device).model(0)


class ARGARCHModel:
    """ARGARCHModel (GARCH.scala:198-260)."""

    def __init__(self, c=0.0, phi=0.0, omega=0.0, alpha=0.0, beta=0.0, jmodel=None, sc=None, device=None):
        self.c, self.phi = float(c), float(phi)
        self.omega, self.alpha, self.beta = float(omega), float(alpha), float(beta)
        self._device = device

    @property
    def _eng(self):
        return _lib.Engine.get(self._device)

    @property
    def _coef(self):
        return np.array([self.c, self.phi, self.omega, self.alpha, self.beta])

    def _apply(self, fn, ts, dest_ts):
        ts = np.asarray(ts, dtype=np.float64).ravel()
        res = fn(ts[None, :], self._coef)[0]
        if dest_ts is None:
            return res
        dest_ts[...] = res
        return dest_ts

    def remove_time_dependent_effects(self, ts, dest_ts=None):
        """removeTimeDependentEffects (GARCH.scala:205-219): the AR(1) residuals standardised by their deviation."""
        return self._apply(self._eng.argarch_remove_effects, ts, dest_ts)

    def add_time_dependent_effects(self, ts, dest_ts=None):
        """addTimeDependentEffects (GARCH.scala:221-236): the model driven by the standardised `ts`."""
        return self._apply(self._eng.argarch_add_effects, ts, dest_ts)

    def sample(self, z):
        """sample(n, rand) (GARCH.scala:238-259) with the gaussians drawn by the caller: z[t] is the t-th
        rand.nextGaussian(). As in the reference the first value is 0.0 and z[0] only feeds the next variance."""
        return self._apply(self._eng.argarch_sample, z, None)
