from . import ARIMA  # noqa: F401
from . import EWMA  # noqa: F401
from . import GARCH  # noqa: F401
from . import ARGARCH  # noqa: F401
from . import Autoregression  # noqa: F401
from . import AutoregressionX  # noqa: F401
from . import RegressionARIMA  # noqa: F401
from . import ARIMAX  # noqa: F401
