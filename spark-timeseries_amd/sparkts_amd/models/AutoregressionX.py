"""MI355X-native mirror of python/sparkts/models/AutoregressionX.py (spark-ts) over the HIP engine.

`fit_model` is AutoregressionX.fitModel (AutoregressionX.scala:48-92): ordinary least squares of y(t) on its own
`y_max_lag` lags, the `x_max_lag` lags of every column of the exogenous matrix `x` and, with `include_original_x`, the
columns' values at t, with an intercept unless `no_intercept`. The regression is commons-math3's QR, run on the device
in the reference's order (csrc/arima_regress.hip). `x` is (T, k), or (N, T, k) in the batched calls when every series
has its own matrix.
"""
import numpy as np

from .. import _lib
from .ARIMA import _EXC, ARIMAFitError


def raise_for_status(status):
    """Raises the exception the reference's regression throws for a per-series status (same classes as ARIMA's)."""
    if status != _lib.ST_OK:
        exc = _EXC.get(int(status), ARIMAFitError)
        e = exc(f"ARX fit failed: status {int(status)} ({_lib.load().arima_status_name(int(status)).decode()})")
        e.status = int(status)
        raise e


class ARXFitBatchResult:
    """Per-series outputs of a batched ARX fit: c (N,), coefficients (N, K), status (N,)."""

    def __init__(self, y_max_lag, x_max_lag, include_original_x, r, device=None):
        self.y_max_lag, self.x_max_lag, self.include_original_x = y_max_lag, x_max_lag, include_original_x
        self.c = r["coef"][:, 0].copy()
        self.coefficients = np.ascontiguousarray(r["coef"][:, 1:])
        self.status = r["status"]
        self._device = device

    def model(self, i):
        raise_for_status(self.status[i])
        return ARXModel(float(self.c[i]), self.coefficients[i], self.y_max_lag, self.x_max_lag,
                        self.include_original_x, device=self._device)

    @property
    def converged(self):
        return self.status == _lib.ST_OK


def fit_models(series, x, y_max_lag, x_max_lag, include_original_x=True, no_intercept=False, device=None):
    """Batched AutoregressionX.fitModel: `series` is (N, T) float64, one row per series; `x` is (T, k) when shared and
    (N, T, k) when per series. Never raises for per-series failures; inspect `.status` (a failed series has NaN
    parameters)."""
    r = _lib.Engine.get(device).arx_fit(series, x, y_max_lag, x_max_lag, include_original_x, no_intercept)
    return ARXFitBatchResult(y_max_lag, x_max_lag, include_original_x, r, device)


def fit_model(y, x, y_max_lag, x_max_lag, include_original_x=True, no_intercept=False, sc=None, device=None):
    """AutoregressionX.fitModel (AutoregressionX.scala:48-68), one series. Raises the reference's exception on
    failure."""
    y = np.asarray(y, dtype=np.float64).ravel()
    return fit_models(y[None, :], np.asarray(x, dtype=np.float64).reshape(y.size, -1), y_max_lag, x_max_lag,
                      include_original_x, no_intercept, device=device).model(0)


def predict_batch(series, x, c, coefficients, y_max_lag, x_max_lag, includes_original_x=True, device=None):
    """Batched ARXModel.predict: c (N,) or a scalar, coefficients (N, K) or (K,), one model per row or one for all:
    (N, T - max(y_max_lag, x_max_lag))."""
    series = np.atleast_2d(np.asarray(series, dtype=np.float64))
    coefficients = np.atleast_2d(np.asarray(coefficients, dtype=np.float64))
    n = series.shape[0]
    coef = np.concatenate([np.broadcast_to(np.asarray(c, dtype=np.float64).reshape(-1, 1), (n, 1)),
                           np.broadcast_to(coefficients, (n, coefficients.shape[1]))], axis=1)
    return _lib.Engine.get(device).arx_predict(series, x, y_max_lag, x_max_lag, includes_original_x, coef)


class ARXModel:
    """ARXModel (AutoregressionX.scala:110-131): intercept `c` and `coefficients` in the order the y lags, then per x
    column its lags, then the non-lagged x columns."""

    def __init__(self, c=0.0, coefficients=(), y_max_lag=0, x_max_lag=0, includes_original_x=True, jmodel=None, sc=None,
                 device=None):
        self.c = float(c)
        self.coefficients = np.atleast_1d(np.asarray(coefficients, dtype=np.float64)).ravel()
        self.y_max_lag, self.x_max_lag, self.includes_original_x = y_max_lag, x_max_lag, includes_original_x
        self._device = device

    def predict(self, y, x):
        """predict(y, x) (:117-130): one value per row of the lagged design, T - max(y_max_lag, x_max_lag) of them."""
        y = np.asarray(y, dtype=np.float64).ravel()
        x = np.asarray(x, dtype=np.float64).reshape(y.size, -1)
        return predict_batch(y[None, :], x, self.c, self.coefficients, self.y_max_lag, self.x_max_lag,
                             self.includes_original_x, device=self._device)[0]
