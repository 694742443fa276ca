from . import ARIMA  # noqa: F401
from . import EWMA  # noqa: F401
from . import GARCH  # noqa: F401
