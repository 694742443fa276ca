"""MI355X-native ARIMAX (models/ARIMAX.scala of spark-ts) over the HIP engine.

`fit_model` is ARIMAX.fitModel (ARIMAX.scala:59-87): an ARIMA(p, d, q) with the columns of `xreg`, their `xreg_max_lag`
lags and, with `include_original_xreg`, their values at t. The start point is an AutoregressionX regression plus the MA
part of Hannan-Rissanen, the optimizer ARIMA's css-cgd; the reference's quirks are kept. The
coefficients are (intercept slot, AR, MA, xreg): 1 + p + q + k * xreg_max_lag (+ k) of them, slot 0 also without an
intercept. `xreg` is (T, k), or (N, T, k) in the batched calls when every series has its own matrix.
"""
import numpy as np

from .. import _lib
from .ARIMA import _EXC, ARIMAFitError, ARIMAModel


def raise_for_status(status):
    """Raises the exception the reference throws for a per-series status (same classes as ARIMA's)."""
    if status != _lib.ST_OK:
        exc = _EXC.get(int(status), ARIMAFitError)
        e = exc(f"ARIMAX fit failed: status {int(status)} ({_lib.load().arima_status_name(int(status)).decode()})")
        e.status = int(status)
        raise e


class ARIMAXFitBatchResult:
    """Per-series outputs of a batched ARIMAX fit: coefficients (N, K'), css_loglik, status, n_eval, n_grad (N,)."""

    def __init__(self, p, d, q, xreg_max_lag, include_original_xreg, include_intercept, r, device=None):
        self.p, self.d, self.q, self.xreg_max_lag = p, d, q, xreg_max_lag
        self.include_original_xreg, self.include_intercept = include_original_xreg, include_intercept
        self.coefficients = r["coef"]
        self.css_loglik = r["ll"]
        self.status = r["status"]
        self.n_eval = r["n_eval"]
        self.n_grad = r["n_grad"]
        self._device = device

    def model(self, i):
        raise_for_status(self.status[i])
        return ARIMAXModel(self.p, self.d, self.q, self.xreg_max_lag, self.coefficients[i], self.include_original_xreg,
                           self.include_intercept, device=self._device)

    @property
    def converged(self):
        return self.status == _lib.ST_OK


def fit_models(p, d, q, series, xreg, xreg_max_lag, include_original_xreg=True, include_intercept=True,
               user_init_params=None, device=None):
    """Batched ARIMAX.fitModel: `series` is (N, T) float64, one row per series; `xreg` is (T, k) when shared and
    (N, T, k) when per series; `user_init_params` (K',) or (N, K') skips the start point. Never raises for per-series
    failures; inspect `.status` (a failed series has NaN coefficients)."""
    r = _lib.Engine.get(device).arimax_fit(series, xreg, p, d, q, xreg_max_lag, include_original_xreg,
                                           include_intercept, user_init_params)
    return ARIMAXFitBatchResult(p, d, q, xreg_max_lag, include_original_xreg, include_intercept, r, device)


def fit_model(p, d, q, ts, xreg, xreg_max_lag, include_original_xreg=True, include_intercept=True,
              user_init_params=None, device=None):
    """ARIMAX.fitModel (ARIMAX.scala:59-87), one series. Raises the reference's exception on failure."""
    ts = np.asarray(ts, dtype=np.float64).ravel()
    return fit_models(p, d, q, ts[None, :], np.asarray(xreg, dtype=np.float64).reshape(ts.size, -1), xreg_max_lag,
                      include_original_xreg, include_intercept, user_init_params, device=device).model(0)


def check_forecast_shape(T, k, n_future, p, d, q, xreg_max_lag):
    """Raises ValueError for the shapes ARIMAXModel.forecast throws for whatever the values are; the C
    ABI returns ARIMA_E_INVALID_ARG for the same."""
    M = max(p, q)
    rows = M + max(n_future - d, 0)
    if min(T, n_future, p, d, q, xreg_max_lag) < 0 or k < 1:
        raise ValueError("negative shape or no xreg column")
    if M == 0:
        raise ValueError("max(p, q) = 0: the reference indexes xregPredictors(-1)")
    if T < d:
        raise ValueError("series shorter than d")
    if rows < xreg_max_lag:
        raise ValueError("fewer differenced xreg rows than xreg_max_lag")
    if rows - xreg_max_lag > M + T - d:
        raise ValueError("more predictor rows than history (nFuture - xreg_max_lag > T)")


def forecast_batch(series, xreg, p, d, q, xreg_max_lag, coefficients, include_original_xreg=True,
                   include_intercept=True, device=None):
    """Batched ARIMAXModel.forecast: `xreg` (nFuture, k) shared or (N, nFuture, k); `coefficients` (K',) or (N, K'):
    (N, T). Shapes the reference throws for raise ValueError (check_forecast_shape)."""
    xs = np.shape(xreg)
    if len(xs) in (2, 3):
        check_forecast_shape(np.shape(series)[-1], xs[-1], xs[-2], p, d, q, xreg_max_lag)
    return _lib.Engine.get(device).arimax_forecast(series, xreg, p, d, q, xreg_max_lag, include_original_xreg,
                                                   include_intercept, coefficients)


class ARIMAXModel:
    """ARIMAXModel (ARIMAX.scala:181-613)."""

    def __init__(self, p=0, d=0, q=0, xreg_max_lag=0, coefficients=(), include_original_xreg=True,
                 include_intercept=True, device=None):
        self.p, self.d, self.q, self.xreg_max_lag = int(p), int(d), int(q), int(xreg_max_lag)
        self.coefficients = np.asarray(coefficients, dtype=np.float64).copy()
        self.include_original_xreg, self.include_intercept = bool(include_original_xreg), bool(include_intercept)
        self._device = device

    def _arima(self):
        """The ARIMA model the effects pair and the log-likelihood read (:266-281, :572-611): `coefficients(intercept
        + j)` over the first I + p + q coefficients."""
        ka = self.p + self.q + (1 if self.include_intercept else 0)
        return ARIMAModel(self.p, self.d, self.q, self.coefficients[:ka], self.include_intercept, device=self._device)

    def forecast(self, ts, xreg):
        """forecast(ts, xreg) (:201-256): nFuture = the rows of xreg; the last len(ts) of the fitted and forecast
        values."""
        ts = np.asarray(ts, dtype=np.float64).ravel()
        xreg = np.asarray(xreg, dtype=np.float64)
        return self.forecast_batch(ts[None, :], xreg[:, None] if xreg.ndim == 1 else xreg)[0]

    def forecast_batch(self, series, xreg):
        return forecast_batch(series, xreg, self.p, self.d, self.q, self.xreg_max_lag, self.coefficients,
                              self.include_original_xreg, self.include_intercept, device=self._device)

    def log_likelihood_css_arma(self, diffedy):
        """logLikelihoodCSSARMA (:266-281) on an already differenced series."""
        return self._arima().log_likelihood_css_arma(diffedy)

    def remove_time_dependent_effects(self, ts, dest_ts=None):
        """removeTimeDependentEffects (:572-587)."""
        return self._arima().remove_time_dependent_effects(ts, dest_ts)

    def add_time_dependent_effects(self, ts, dest_ts=None):
        """addTimeDependentEffects (:599-611)."""
        return self._arima().add_time_dependent_effects(ts, dest_ts)
