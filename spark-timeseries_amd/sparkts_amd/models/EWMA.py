"""MI355X-native mirror of python/sparkts/models/EWMA.py (spark-ts) over the HIP engine.

Exponentially weighted moving average (simple exponential smoothing): S_t = a * X_t + (1 - a) * S_{t-1} with S_0 = X_0
(EWMA.scala:135-143). `fit_model` is EWMA.fitModel (EWMA.scala:45-69): the smoothing parameter that minimises the sum
of squared one-step errors, by commons-math3's Fletcher-Reeves conjugate gradient from 0.94, unbounded -- the result
should be sanity checked as the reference says. `sc` is accepted and ignored (there is no JVM). `fit_models` is the
batched form (one ABI call per partition bucket).
"""
import numpy as np

from .. import _lib
from .ARIMA import _EXC, ARIMAFitError


def raise_for_status(status):
    """Raises the exception the reference's optimizer throws for a per-series status (same classes as ARIMA's)."""
    if status != _lib.ST_OK:
        exc = _EXC.get(int(status), ARIMAFitError)
        e = exc(f"EWMA fit failed: status {int(status)} ({_lib.load().arima_status_name(int(status)).decode()})")
        e.status = int(status)
        raise e


class EWMAFitBatchResult:
    """Per-series outputs of a batched EWMA fit (the arrays arima_ewma_fit_batch fills)."""

    def __init__(self, r, device=None):
        self.smoothing = r["smoothing"]
        self.sse = r["sse"]
        self.status = r["status"]
        self.n_eval = r["n_eval"]
        self.n_grad = r["n_grad"]
        self._device = device

    def model(self, i):
        raise_for_status(self.status[i])
        return EWMAModel(float(self.smoothing[i]), device=self._device)

    @property
    def converged(self):
        return self.status == _lib.ST_OK


def fit_models(series, device=None):
    """Batched EWMA.fitModel: `series` is (N, T) float64, one row per series. Never raises for per-series failures;
    inspect `.status` (a failed series has a NaN smoothing)."""
    return EWMAFitBatchResult(_lib.Engine.get(device).ewma_fit_batch(series), device)


def fit_model(ts, sc=None, device=None):
    """EWMA.fitModel (EWMA.scala:45-69), one series. Raises the reference's exception on failure."""
    ts = np.asarray(ts, dtype=np.float64).ravel()
    return fit_models(ts[None, :], device=device).model(0)


class EWMAModel:
    """EWMAModel (EWMA.scala:72-144) with the reference Python binding's names."""

    def __init__(self, smoothing=0.0, jmodel=None, sc=None, device=None):
        self.smoothing = float(smoothing)
        self._device = device

    @property
    def _eng(self):
        return _lib.Engine.get(self._device)

    def _apply(self, fn, ts, dest_ts):
        ts = np.asarray(ts, dtype=np.float64).ravel()
        res = fn(ts[None, :], self.smoothing)[0]
        if dest_ts is None:
            return res
        dest_ts[...] = res          # the reference fills destTs and returns it
        return dest_ts

    def sse(self, ts):
        """sse (EWMA.scala:81-96): the sum of squared one-step-ahead errors."""
        return float(self._eng.ewma_sse(np.asarray(ts, dtype=np.float64).ravel()[None, :], self.smoothing)[0])

    def gradient(self, ts):
        """gradient (EWMA.scala:102-123): d sse / d smoothing."""
        return float(self._eng.ewma_gradient(np.asarray(ts, dtype=np.float64).ravel()[None, :], self.smoothing)[0])

    def remove_time_dependent_effects(self, ts, dest_ts=None):
        """removeTimeDependentEffects (EWMA.scala:125-133): the series whose smoothing gives `ts`."""
        return self._apply(self._eng.ewma_remove_effects, ts, dest_ts)

    def add_time_dependent_effects(self, ts, dest_ts=None):
        """addTimeDependentEffects (EWMA.scala:135-143): `ts` smoothed."""
        return self._apply(self._eng.ewma_add_effects, ts, dest_ts)
