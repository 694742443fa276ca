"""MI355X-native mirror of python/sparkts/models/RegressionARIMA.py (spark-ts) over the HIP engine.

`fit_cochrane_orcutt` is RegressionARIMA.fitCochraneOrcutt (RegressionARIMA.scala:83-160): a regression of the series
on the columns of `regressors`, with an intercept and AR(1) errors, by the iterated Cochrane-Orcutt procedure. The
whole iteration of a series runs on the device in the reference's order (k_cochrane_orcutt, csrc/arima_regress.hip).
`regressors` is (T, k), or (N, T, k) in the batched call when every series has its own matrix.
"""
import numpy as np

from .. import _lib
from .ARIMA import _EXC, ARIMAFitError, UnsupportedOperationException


def raise_for_status(status):
    """Raises the exception the reference's regression throws for a per-series status (same classes as ARIMA's)."""
    if status != _lib.ST_OK:
        exc = _EXC.get(int(status), ARIMAFitError)
        e = exc(f"RegressionARIMA fit failed: status {int(status)} "
                f"({_lib.load().arima_status_name(int(status)).decode()})")
        e.status = int(status)
        raise e


class RegressionARIMAFitBatchResult:
    """Per-series outputs of a batched Cochrane-Orcutt fit: regression_coeff (N, 1 + k), the intercept first; rho (N,),
    the AR(1) coefficient of the errors (0.0 for a series that never iterated); n_iter (N,); status (N,)."""

    def __init__(self, r):
        self.regression_coeff = r["coef"]
        self.rho = r["rho"]
        self.n_iter = r["n_iter"]
        self.status = r["status"]

    def model(self, i):
        raise_for_status(self.status[i])
        return RegressionARIMAModel(self.regression_coeff[i], (1, 0, 0), [self.rho[i]])

    @property
    def converged(self):
        return self.status == _lib.ST_OK


def fit_models(series, regressors, max_iter=10, device=None):
    """Batched RegressionARIMA.fitCochraneOrcutt: `series` is (N, T) float64, one row per series; `regressors` is
    (T, k) when shared and (N, T, k) when per series. Never raises for per-series failures; inspect `.status` (a failed
    series has NaN parameters)."""
    return RegressionARIMAFitBatchResult(_lib.Engine.get(device).regarima_co_fit(series, regressors, max_iter))


def fit_cochrane_orcutt(ts, regressors, max_iter=10, device=None):
    """RegressionARIMA.fitCochraneOrcutt (RegressionARIMA.scala:83-160), one series. Raises the reference's exception
    on failure."""
    ts = np.asarray(ts, dtype=np.float64).ravel()
    regressors = np.asarray(regressors, dtype=np.float64)
    if regressors.ndim == 1:
        regressors = regressors[:, None]
    if regressors.ndim != 2 or regressors.shape[0] != ts.size:
        raise ValueError(f"regressors must have one row per time point: {regressors.shape} against {ts.size}")
    return fit_models(ts[None, :], regressors, max_iter, device=device).model(0)


def fit_model(ts, regressors, method, *optimization_args, device=None):
    """RegressionARIMA.fitModel (RegressionARIMA.scala:35-59): `method` "cochrane-orcutt", with at most one
    optimization argument, the maximum number of iterations."""
    if method != "cochrane-orcutt":
        e = UnsupportedOperationException(f'Regression ARIMA method "{method}" not defined.')
        e.status = _lib.ST_UNSUPPORTED_METHOD
        raise e
    if not optimization_args:
        return fit_cochrane_orcutt(ts, regressors, device=device)
    if isinstance(optimization_args[0], bool) or not isinstance(optimization_args[0], (int, np.integer)):
        raise ValueError("Maximum iteration parameter to Cochrane-Orcutt must be integer")
    if len(optimization_args) > 1:
        raise ValueError("Number of Cochrane-Orcutt arguments can't exceed 3")
    return fit_cochrane_orcutt(ts, regressors, int(optimization_args[0]), device=device)


class RegressionARIMAModel:
    """RegressionARIMAModel (RegressionARIMA.scala:185-201): `regression_coeff`, the intercept first; `arima_orders`
    (p, d, q) of the error structure; `arima_coeff`, its p + d + q terms."""

    def __init__(self, regression_coeff, arima_orders, arima_coeff, jmodel=None, sc=None):
        self.regression_coeff = np.atleast_1d(np.asarray(regression_coeff, dtype=np.float64)).ravel()
        self.arima_orders = np.atleast_1d(np.asarray(arima_orders, dtype=np.int32)).ravel()
        self.arima_coeff = np.atleast_1d(np.asarray(arima_coeff, dtype=np.float64)).ravel()

    def add_time_dependent_effects(self, ts, dest=None):
        """The reference throws UnsupportedOperationException (:190-194)."""
        raise NotImplementedError("RegressionARIMAModel.addTimeDependentEffects")

    def remove_time_dependent_effects(self, ts, dest=None):
        """The reference throws UnsupportedOperationException (:196-200)."""
        raise NotImplementedError("RegressionARIMAModel.removeTimeDependentEffects")
