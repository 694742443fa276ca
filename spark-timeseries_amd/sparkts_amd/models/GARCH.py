"""MI355X-native mirror of python/sparkts/models/GARCH.py (spark-ts) over the HIP engine.

GARCH(1,1): h_t = omega + alpha * eta_{t-1}^2 + beta * h_{t-1}. `fit_model` is GARCH.fitModel (GARCH.scala:33-53):
commons-math3's Fletcher-Reeves conjugate gradient from (.2, .2, .2) on GARCHModel.logLikelihood. Two properties of the
reference are reproduced, not repaired, so that this is a drop-in: no GoalType is passed, which makes commons maximise;
and GARCHModel.gradient returns (alpha, beta, omega) halves while the parameters are (omega, alpha, beta), so each
parameter moves along another one's derivative. `sc` is accepted and ignored. `sample` takes the gaussians
from the caller (the reference draws them from a commons RandomGenerator).
"""
import numpy as np

from .. import _lib
from .ARIMA import _EXC, ARIMAFitError


def raise_for_status(status):
    """Raises the exception the reference's optimizer throws for a per-series status (same classes as ARIMA's)."""
    if status != _lib.ST_OK:
        exc = _EXC.get(int(status), ARIMAFitError)
        e = exc(f"GARCH fit failed: status {int(status)} ({_lib.load().arima_status_name(int(status)).decode()})")
        e.status = int(status)
        raise e


class GARCHFitBatchResult:
    """Per-series outputs of a batched GARCH fit (the arrays arima_garch_fit_batch fills)."""

    def __init__(self, r, device=None):
        self.coefficients = r["coef"]            # (N, 3): omega, alpha, beta
        self.log_likelihood = r["ll"]
        self.status = r["status"]
        self.n_eval = r["n_eval"]
        self.n_grad = r["n_grad"]
        self._device = device

    omega = property(lambda self: self.coefficients[:, 0])
    alpha = property(lambda self: self.coefficients[:, 1])
    beta = property(lambda self: self.coefficients[:, 2])

    def model(self, i):
        raise_for_status(self.status[i])
        return GARCHModel(*(float(v) for v in self.coefficients[i]), device=self._device)

    @property
    def converged(self):
        return self.status == _lib.ST_OK


def fit_models(series, device=None):
    """Batched GARCH.fitModel: `series` is (N, T) float64, one row per series. Never raises for per-series failures;
    inspect `.status` (a failed series has NaN parameters)."""
    return GARCHFitBatchResult(_lib.Engine.get(device).garch_fit_batch(series), device)


def fit_model(ts, sc=None, device=None):
    """GARCH.fitModel (GARCH.scala:33-53), one series. Raises the reference's exception on failure."""
    ts = np.asarray(ts, dtype=np.float64).ravel()
    return fit_models(ts[None, :], device=device).model(0)


class GARCHModel:
    """GARCHModel (GARCH.scala:73-178) with the reference Python binding's names."""

    def __init__(self, omega=0.0, alpha=0.0, beta=0.0, jmodel=None, sc=None, device=None):
        self.omega, self.alpha, self.beta = float(omega), float(alpha), float(beta)
        self._device = device

    @property
    def _eng(self):
        return _lib.Engine.get(self._device)

    @property
    def _coef(self):
        return np.array([self.omega, self.alpha, self.beta])

    def gradient(self, ts):
        """gradient (GARCH.scala:96-115): a 3-element array for the alpha, beta and omega parameters, in that order."""
        return self._eng.garch_gradient(np.asarray(ts, dtype=np.float64).ravel()[None, :], self._coef)[0]

    def log_likelihood(self, ts):
        """logLikelihood (GARCH.scala:82-88)."""
        return float(self._eng.garch_loglik(np.asarray(ts, dtype=np.float64).ravel()[None, :], self._coef)[0])

    def _apply(self, fn, ts, dest_ts):
        ts = np.asarray(ts, dtype=np.float64).ravel()
        res = fn(ts[None, :], self._coef)[0]
        if dest_ts is None:
            return res
        dest_ts[...] = res
        return dest_ts

    def remove_time_dependent_effects(self, ts, dest_ts=None):
        """removeTimeDependentEffects (GARCH.scala:131-145): `ts` standardised by its conditional deviation."""
        return self._apply(self._eng.garch_remove_effects, ts, dest_ts)

    def add_time_dependent_effects(self, ts, dest_ts=None):
        """addTimeDependentEffects (GARCH.scala:147-162): the model driven by the standardised `ts`."""
        return self._apply(self._eng.garch_add_effects, ts, dest_ts)

    def sample(self, z):
        """sample(n, rand) (GARCH.scala:164-185) with the gaussians drawn by the caller: z[t] is the t-th
        rand.nextGaussian(). As in the reference the first value is 0.0 and z[0] only feeds the next variance."""
        return self._apply(self._eng.garch_sample, z, None)
