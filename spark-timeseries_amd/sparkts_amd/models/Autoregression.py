"""MI355X-native mirror of python/sparkts/models/Autoregression.py (spark-ts) over the HIP engine.

`fit_model` is Autoregression.fitModel (Autoregression.scala:28-53): ordinary least squares of ts(t) on its `max_lag`
lags, with an intercept unless `no_intercept`. It runs the engine's AR-only fit path (arima_fit_batch with d = q = 0).
ARModel's TimeSeriesModel pair uses, at step i < p, only the lags that exist, which ARIMAModel's pair does not.
"""
import numpy as np

from .. import _lib
from .ARIMA import _EXC, ARIMAFitError

MAX_LAG = _lib.AR_MAX_LAG


def raise_for_status(status):
    """Raises the exception the reference's regression throws for a per-series status (same classes as ARIMA's)."""
    if status != _lib.ST_OK:
        exc = _EXC.get(int(status), ARIMAFitError)
        e = exc(f"AR fit failed: status {int(status)} ({_lib.load().arima_status_name(int(status)).decode()})")
        e.status = int(status)
        raise e


class ARFitBatchResult:
    """Per-series outputs of a batched AR fit: c (N,), coefficients (N, max_lag), status (N,)."""

    def __init__(self, max_lag, no_intercept, r, device=None):
        self.max_lag, self.no_intercept = max_lag, no_intercept
        coef = r["coef"]
        self.c = np.zeros(coef.shape[0]) if no_intercept else coef[:, 0].copy()
        self.coefficients = np.ascontiguousarray(coef if no_intercept else coef[:, 1:])
        self.c[r["status"] != _lib.ST_OK] = np.nan
        self.status = r["status"]
        self._device = device

    def model(self, i):
        raise_for_status(self.status[i])
        return ARModel(float(self.c[i]), self.coefficients[i], device=self._device)

    @property
    def converged(self):
        return self.status == _lib.ST_OK


def fit_models(series, max_lag=1, no_intercept=False, device=None):
    """Batched Autoregression.fitModel: `series` is (N, T) float64, one row per series. Never raises for per-series
    failures; inspect `.status` (a failed series has NaN parameters)."""
    r = _lib.Engine.get(device).fit_batch(series, max_lag, 0, 0, not no_intercept)
    return ARFitBatchResult(max_lag, no_intercept, r, device)


def fit_model(ts, max_lag=1, no_intercept=False, sc=None, device=None):
    """Autoregression.fitModel (Autoregression.scala:38-53), one series. Raises the reference's exception on failure."""
    ts = np.asarray(ts, dtype=np.float64).ravel()
    return fit_models(ts[None, :], max_lag, no_intercept, device=device).model(0)


class ARModel:
    """ARModel (Autoregression.scala:56-96): intercept `c` and `coefficients` phi_1 .. phi_p, 1 <= p <= 20."""

    def __init__(self, c=0.0, coefficients=(), jmodel=None, sc=None, device=None):
        self.c = float(c)
        self.coefficients = np.atleast_1d(np.asarray(coefficients, dtype=np.float64)).ravel()
        self._device = device

    @property
    def _eng(self):
        return _lib.Engine.get(self._device)

    def _apply(self, fn, ts, dest_ts):
        ts = np.asarray(ts, dtype=np.float64).ravel()
        res = fn(ts[None, :], self.coefficients.size, np.concatenate([[self.c], self.coefficients]))[0]
        if dest_ts is None:
            return res
        dest_ts[...] = res
        return dest_ts

    def remove_time_dependent_effects(self, ts, dest_ts=None):
        """removeTimeDependentEffects (Autoregression.scala:60-75): the residuals of `ts` under the model."""
        return self._apply(self._eng.ar_remove_effects, ts, dest_ts)

    def add_time_dependent_effects(self, ts, dest_ts=None):
        """addTimeDependentEffects (Autoregression.scala:77-90): the model driven by the innovations `ts`."""
        return self._apply(self._eng.ar_add_effects, ts, dest_ts)

    def sample(self, z):
        """sample(n, rand) (Autoregression.scala:92-95) with the gaussians drawn by the caller: the model driven by z."""
        return self._apply(self._eng.ar_add_effects, z, None)
