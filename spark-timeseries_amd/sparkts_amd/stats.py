"""Batched mirrors of the reference's residual tests (TimeSeriesStatisticalTests.scala, UnivariateTimeSeries.scala) over
the rows of an (N, T) array, one device call each. A 1-D input is one row. The Breusch-Godfrey and Breusch-Pagan tests
take the regressor matrix of the model the residuals came from: `factors` is (T, k) when every row shares it and
(N, T, k) when every row has its own."""
from . import _lib


def autocorr(rows, num_lags, device=None):
    """UnivariateTimeSeries.autocorr (UnivariateTimeSeries.scala:70-96) per row: (N, num_lags), lag i at column i - 1."""
    return _lib.Engine.get(device).diagnostics(rows, num_lags, ("acf",))["acf"]


def dwtest(rows, device=None):
    """TimeSeriesStatisticalTests.dwtest (:251-262) per row: the Durbin-Watson statistic, (N,)."""
    return _lib.Engine.get(device).diagnostics(rows, 0, ("dw",))["dw"]


def lbtest(rows, max_lag, device=None):
    """TimeSeriesStatisticalTests.lbtest (:298-307) per row: (statistic, p-value), each (N,)."""
    r = _lib.Engine.get(device).diagnostics(rows, max_lag, ("lb_stat", "lb_pvalue"))
    return r["lb_stat"], r["lb_pvalue"]


def bgtest(residuals, factors, max_lag, device=None):
    """TimeSeriesStatisticalTests.bgtest (:276-288) per row: (statistic, p-value), each (N,). A row the reference
    would throw for (too short for the auxiliary regression, a singular design) has NaN in both."""
    r = _lib.Engine.get(device).bgtest(residuals, factors, max_lag)
    return r["stat"], r["pvalue"]


def bptest(residuals, factors, device=None):
    """TimeSeriesStatisticalTests.bptest (:320-329) per row: (statistic, p-value), each (N,); NaN where the reference
    would throw."""
    r = _lib.Engine.get(device).bptest(residuals, factors)
    return r["stat"], r["pvalue"]
