"""sparkts_amd — MI355X-native drop-in for spark-ts's ARIMA CSS-CGD fit path (ARIMA.fitModel under mapSeries).

Host-side mirror of the reference's Python API (python/sparkts/) over the C ABI of libsparkts_arima.so.
"""
from . import _lib  # noqa: F401
from . import stats  # noqa: F401
from .models import ARGARCH, ARIMA, EWMA, GARCH, Autoregression  # noqa: F401
from .timeseriesrdd import (arima_diagnostics_partition, arima_residuals_partition,  # noqa: F401
                            fit_argarch_partition, fit_arima_partition, fit_ewma_partition,
                            fit_garch_partition,
                            map_series_fit_arima)

__version__ = "0.1.0"
