"""ctypes binding of libsparkts_arima.so (the C ABI declared in include/sparkts_arima.h).

The product path has no CPU fallback: if the HIP library is missing or no GPU is visible, every compute call
raises. Only symbol loading works without a GPU (used by the CPU test-suite to check the exported ABI).
"""
import ctypes
import os
import threading

import numpy as np

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # spark-timeseries_amd/
LIB_PATH = os.environ.get("SPARKTS_ARIMA_LIB", os.path.join(_PKG_ROOT, "libsparkts_arima.so"))

ARIMA_OK = 0
ARIMA_E_INVALID_ARG = -1
ARIMA_E_UNSUPPORTED = -2
ARIMA_E_DEVICE = -3
ARIMA_E_OOM = -4

ST_OK = 0
ST_MAX_EVAL = 1
ST_BRACKET_MAX_EVAL = 2
ST_MAX_ITER = 3
ST_SINGULAR = 4
ST_NOT_ENOUGH_DATA = 5
ST_NO_DATA = 6
ST_BAD_INTERVAL = 7
ST_ZERO_PARAMS = 8
ST_UNSUPPORTED_METHOD = 9
ST_SERIES_TOO_SHORT = 10
ST_NOT_STATIONARY = 11      # autoFit: no d <= max_d passes KPSS
ST_NO_MODEL = 12            # autoFit: no candidate qualified
ST_TOO_FEW_PARAMS = 14      # css-bobyqa needs >= 2 parameters (NumberIsTooSmallException)

METHOD_CSS_CGD = 0
METHOD_CSS_BOBYQA = 1
METHODS = {"css-cgd": METHOD_CSS_CGD, "css-bobyqa": METHOD_CSS_BOBYQA}

FLAG_STATIONARY = 1
FLAG_INVERTIBLE = 2

# arima_set_option("smear", .) default: Breeze 0.12's element-wise copy of the overlapping row slice at
# ARIMA.scala:526; 0 selects the memmove-like row shift.
DEFAULT_SMEAR = 1

# every symbol include/sparkts_arima.h declares (checked by tests/test_abi.py)
EXPORTED = [
    "arima_create", "arima_destroy", "arima_last_error", "arima_status_name", "arima_num_params",
    "arima_get_last_stats", "arima_set_option", "arima_get_option", "arima_fit_batch", "arima_fit_batch_device",
    "arima_difference_batch", "arima_inverse_difference_batch", "arima_css_loglik_batch",
    "arima_css_gradient_batch", "arima_hannan_rissanen_batch", "arima_forecast_batch", "arima_model_flags_batch",
    "arima_sample_batch_device", "arima_order_search_batch", "arima_order_search_batch_device",
    "arima_forecast_batch_device", "arima_synchronize", "arima_autofit_batch", "arima_autofit_batch_device",
    "arima_kpss_batch", "arima_remove_effects_batch", "arima_remove_effects_batch_device",
    "arima_add_effects_batch", "arima_add_effects_batch_device",
    "arima_diagnostics_batch", "arima_diagnostics_batch_device", "arima_residual_diagnostics_batch",
    "arima_residual_diagnostics_batch_device",
    "arima_ewma_fit_batch", "arima_ewma_fit_batch_device", "arima_garch_fit_batch", "arima_garch_fit_batch_device",
    "arima_ewma_sse_batch", "arima_ewma_gradient_batch", "arima_garch_loglik_batch", "arima_garch_gradient_batch",
    "arima_ewma_remove_effects_batch", "arima_ewma_add_effects_batch", "arima_garch_remove_effects_batch",
    "arima_garch_add_effects_batch", "arima_ewma_remove_effects_batch_device", "arima_ewma_add_effects_batch_device",
    "arima_garch_remove_effects_batch_device", "arima_garch_add_effects_batch_device",
    "arima_get_last_model_fit_stats",
    "arima_argarch_fit_batch", "arima_argarch_fit_batch_device", "arima_argarch_remove_effects_batch",
    "arima_argarch_add_effects_batch", "arima_argarch_remove_effects_batch_device",
    "arima_argarch_add_effects_batch_device", "arima_ar_remove_effects_batch", "arima_ar_add_effects_batch",
    "arima_ar_remove_effects_batch_device", "arima_ar_add_effects_batch_device", "arima_garch_sample_batch",
    "arima_argarch_sample_batch", "arima_garch_sample_batch_device", "arima_argarch_sample_batch_device",
    "arima_arx_num_coef", "arima_arx_fit_batch", "arima_arx_fit_batch_device", "arima_arx_predict_batch",
    "arima_arx_predict_batch_device", "arima_bgtest_batch", "arima_bgtest_batch_device", "arima_bptest_batch",
    "arima_bptest_batch_device", "arima_regarima_co_fit_batch", "arima_regarima_co_fit_batch_device",
    "arima_arimax_num_coef", "arima_arimax_fit_batch", "arima_arimax_fit_batch_device", "arima_arimax_forecast_batch",
    "arima_arimax_forecast_batch_device",
]

# the small models (EWMA.scala, GARCH.scala): parameters per series; ARGARCH's are (c, phi, omega, alpha, beta)
MODEL_PARAMS = {"ewma": 1, "garch": 3, "argarch": 5}
AR_MAX_LAG = 20             # the library's order limit (ARModel's pair)


class FitStats(ctypes.Structure):
    _fields_ = [("n_series", ctypes.c_int64), ("f_passes", ctypes.c_int64), ("g_passes", ctypes.c_int64),
                ("hr_passes", ctypes.c_int64), ("n_eval", ctypes.c_int64), ("n_grad", ctypes.c_int64),
                ("flops", ctypes.c_double), ("ms_difference", ctypes.c_double), ("ms_hr_init", ctypes.c_double),
                ("ms_cg_fit", ctypes.c_double), ("ms_total", ctypes.c_double),
                ("wave_f_passes", ctypes.c_int64), ("wave_g_passes", ctypes.c_int64), ("grid_blocks", ctypes.c_int64),
                ("spec_hits", ctypes.c_int64), ("wave_multi_passes", ctypes.c_int64), ("spec_chains", ctypes.c_int64),
                ("express_blocks", ctypes.c_int64), ("express_series", ctypes.c_int64),
                ("express_f_passes", ctypes.c_int64), ("express_g_passes", ctypes.c_int64),
                ("fault", ctypes.c_int64), ("fault_info", ctypes.c_int64 * 5),
                ("diag", ctypes.c_int64 * 6), ("ride_passes", ctypes.c_int64), ("series_done", ctypes.c_int64),
                ("express_pit_passes", ctypes.c_int64), ("express_pit_sweeps", ctypes.c_int64),
                ("express_pit_g_passes", ctypes.c_int64), ("wave_chains", ctypes.c_int64),
                ("low_util_passes", ctypes.c_int64), ("diag_step_cycles", ctypes.c_int64),
                ("diag_refill_cycles", ctypes.c_int64), ("merge_series", ctypes.c_int64),
                ("merge_waves", ctypes.c_int64), ("skipped_g", ctypes.c_int64)]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["diag"] = list(self.diag)
        d["fault_info"] = list(self.fault_info)
        return d


class ModelFitStats(ctypes.Structure):
    """arima_model_fit_stats: the EWMA / GARCH fit kernel's round counters."""
    _fields_ = [("n_series", ctypes.c_int64), ("wave_passes", ctypes.c_int64), ("lane_passes", ctypes.c_int64),
                ("max_wave_passes", ctypes.c_int64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class EngineError(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()
_dp = ctypes.POINTER(ctypes.c_double)
_i32p = ctypes.POINTER(ctypes.c_int32)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_vp = ctypes.c_void_p
_i32, _i64, _f64, _u64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_uint64


def _single_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64/libhsa-runtime64 (same SONAME as /opt/rocm's). If this
    library were loaded first, a later `import torch` would map a SECOND HIP runtime into the process and torch
    would see no GPU. Importing torch first makes the dynamic loader bind this library to torch's runtime, so a
    process that also uses torch (bench.py's torch.distributed plumbing, tests) has exactly one HIP runtime."""
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def load():
    """Load the shared library (no GPU needed). Raises if it is missing."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        _single_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise EngineError(f"HIP library not built: {LIB_PATH} (run `python -c 'import __graft_entry__ as g; "
                              f"g.build()'` or `make -C spark-timeseries_amd/csrc`)")
        L = ctypes.CDLL(LIB_PATH)
        H = ctypes.c_void_p
        L.arima_create.argtypes = [ctypes.c_int, ctypes.POINTER(H)]
        L.arima_destroy.argtypes = [H]
        L.arima_last_error.argtypes = [H]
        L.arima_last_error.restype = ctypes.c_char_p
        L.arima_status_name.argtypes = [ctypes.c_int]
        L.arima_status_name.restype = ctypes.c_char_p
        L.arima_num_params.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.arima_get_last_stats.argtypes = [H, ctypes.POINTER(FitStats)]
        L.arima_set_option.argtypes = [H, ctypes.c_char_p, _i64]
        L.arima_get_option.argtypes = [H, ctypes.c_char_p, ctypes.POINTER(_i64)]
        L.arima_synchronize.argtypes = [H]
        L.arima_fit_batch.argtypes = [H, _dp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _dp, _dp, _dp, _i32p,
                                      _i32p, _i32p, _u8p]
        L.arima_fit_batch_device.argtypes = [H, _vp, _i64, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp,
                                             _vp, _vp, _vp, _vp, _vp]
        L.arima_difference_batch.argtypes = [H, _dp, _i64, _i32, _i32, _dp]
        L.arima_inverse_difference_batch.argtypes = [H, _dp, _i64, _i32, _i32, _dp]
        L.arima_css_loglik_batch.argtypes = [H, _dp, _i64, _i32, _i32, _i32, _i32, _i32, _dp, _dp]
        L.arima_css_gradient_batch.argtypes = [H, _dp, _i64, _i32, _i32, _i32, _i32, _dp, _dp]
        L.arima_hannan_rissanen_batch.argtypes = [H, _dp, _i64, _i32, _i32, _i32, _i32, _dp, _i32p]
        L.arima_forecast_batch.argtypes = [H, _dp, _i64, _i32, _i32, _i32, _i32, _i32, _dp, _i32, _dp]
        L.arima_model_flags_batch.argtypes = [H, _dp, _i64, _i32, _i32, _i32, _u8p]
        L.arima_sample_batch_device.argtypes = [H, _vp, _i64, _i32, _i64, _i32, _i32, _i32, _i32, _dp, _f64, _u64,
                                                _i64, _vp]
        L.arima_forecast_batch_device.argtypes = [H, _vp, _i64, _i32, _i64, _i32, _i32, _i32, _i32, _vp, _i32, _vp,
                                                  _i64, _vp]
        L.arima_order_search_batch.argtypes = [H, _dp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32p, _dp, _dp]
        L.arima_order_search_batch_device.argtypes = [H, _vp, _i64, _i32, _i64, _i32, _i32, _i32, _i32, _i32, _vp,
                                                      _vp, _vp, _vp]
        L.arima_autofit_batch.argtypes = [H, _dp, _i64, _i32, _i32, _i32, _i32, _i32p, _dp, _dp, _i32p, _i32p]
        L.arima_autofit_batch_device.argtypes = [H, _vp, _i64, _i32, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp,
                                                 _vp]
        L.arima_kpss_batch.argtypes = [H, _dp, _i64, _i32, _dp, _i32p]
        for fn in (L.arima_remove_effects_batch, L.arima_add_effects_batch):
            fn.argtypes = [H, _dp, _i64, _i32, _i32, _i32, _i32, _i32, _dp, _dp]
        for fn in (L.arima_remove_effects_batch_device, L.arima_add_effects_batch_device):
            fn.argtypes = [H, _vp, _i64, _i32, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _i64, _vp]
        L.arima_diagnostics_batch.argtypes = [H, _dp, _i64, _i32, _i32, _dp, _dp, _dp, _dp]
        L.arima_diagnostics_batch_device.argtypes = [H, _vp, _i64, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp]
        L.arima_residual_diagnostics_batch.argtypes = [H, _dp, _i64, _i32, _i32, _i32, _i32, _i32, _dp, _i32, _dp, _dp,
                                                       _dp, _dp]
        L.arima_residual_diagnostics_batch_device.argtypes = [H, _vp, _i64, _i32, _i64, _i32, _i32, _i32, _i32, _vp,
                                                              _i32, _vp, _vp, _vp, _vp, _vp]
        for m in ("ewma", "garch", "argarch"):
            getattr(L, f"arima_{m}_fit_batch").argtypes = [H, _dp, _i64, _i32, _dp, _dp, _i32p, _i32p, _i32p]
            getattr(L, f"arima_{m}_fit_batch_device").argtypes = [H, _vp, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp]
            for d in ("remove", "add"):
                getattr(L, f"arima_{m}_{d}_effects_batch").argtypes = [H, _dp, _i64, _i32, _dp, _dp]
                getattr(L, f"arima_{m}_{d}_effects_batch_device").argtypes = [H, _vp, _i64, _i32, _i64, _vp, _vp, _i64,
                                                                             _vp]
        for fn in (L.arima_ewma_sse_batch, L.arima_ewma_gradient_batch, L.arima_garch_loglik_batch,
                   L.arima_garch_gradient_batch):
            fn.argtypes = [H, _dp, _i64, _i32, _dp, _dp]
        L.arima_get_last_model_fit_stats.argtypes = [H, ctypes.POINTER(ModelFitStats)]
        for d in ("remove", "add"):
            getattr(L, f"arima_ar_{d}_effects_batch").argtypes = [H, _dp, _i64, _i32, _i32, _dp, _dp]
            getattr(L, f"arima_ar_{d}_effects_batch_device").argtypes = [H, _vp, _i64, _i32, _i64, _i32, _vp, _vp, _i64,
                                                                        _vp]
        for m in ("garch", "argarch"):
            getattr(L, f"arima_{m}_sample_batch").argtypes = [H, _dp, _i64, _i32, _dp, _dp]
            getattr(L, f"arima_{m}_sample_batch_device").argtypes = [H, _vp, _i64, _i32, _i64, _vp, _vp, _i64, _vp]
        L.arima_arx_num_coef.argtypes = [_i32, _i32, _i32, _i32]
        L.arima_arx_fit_batch.argtypes = [H, _dp, _i64, _i32, _dp, _i64, _i32, _i32, _i32, _i32, _i32, _dp, _i32p]
        L.arima_arx_fit_batch_device.argtypes = [H, _vp, _i64, _i32, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp,
                                                 _vp, _vp]
        L.arima_arx_predict_batch.argtypes = [H, _dp, _i64, _i32, _dp, _i64, _i32, _i32, _i32, _i32, _dp, _dp]
        L.arima_arx_predict_batch_device.argtypes = [H, _vp, _i64, _i32, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _vp,
                                                     _vp, _i64, _vp]
        L.arima_bgtest_batch.argtypes = [H, _dp, _i64, _i32, _dp, _i64, _i32, _i32, _dp, _dp, _i32p]
        L.arima_bgtest_batch_device.argtypes = [H, _vp, _i64, _i32, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp]
        L.arima_bptest_batch.argtypes = [H, _dp, _i64, _i32, _dp, _i64, _i32, _dp, _dp, _i32p]
        L.arima_bptest_batch_device.argtypes = [H, _vp, _i64, _i32, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _vp]
        L.arima_regarima_co_fit_batch.argtypes = [H, _dp, _i64, _i32, _dp, _i64, _i32, _i32, _dp, _dp, _i32p, _i32p]
        L.arima_regarima_co_fit_batch_device.argtypes = [H, _vp, _i64, _i32, _i64, _vp, _i64, _i32, _i32, _vp, _vp,
                                                         _vp, _vp, _vp]
        L.arima_arimax_num_coef.argtypes = [_i32, _i32, _i32, _i32, _i32]
        L.arima_arimax_fit_batch.argtypes = [H, _dp, _i64, _i32, _dp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                             _dp, _dp, _dp, _i32p, _i32p, _i32p]
        L.arima_arimax_fit_batch_device.argtypes = [H, _vp, _i64, _i32, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _i32,
                                                    _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        L.arima_arimax_forecast_batch.argtypes = [H, _dp, _i64, _i32, _dp, _i64, _i32, _i32, _i32, _i32, _i32, _i32,
                                                  _i32, _i32, _dp, _dp]
        L.arima_arimax_forecast_batch_device.argtypes = [H, _vp, _i64, _i32, _i64, _vp, _i64, _i32, _i32, _i32, _i32,
                                                         _i32, _i32, _i32, _i32, _vp, _vp, _i64, _vp]
        _lib = L
        return L


def _ptr(a, t=_dp):
    return a.ctypes.data_as(t) if a is not None else None


class Engine:
    """One handle per device (arima_create). Thread-safe: the library serialises calls per handle."""

    _engines = {}

    def __init__(self, device=0):
        self.L = load()
        h = ctypes.c_void_p()
        rc = self.L.arima_create(int(device), ctypes.byref(h))
        if rc != ARIMA_OK:
            raise EngineError(f"arima_create(device={device}) failed with {rc}: no usable HIP device")
        self.h = h
        self.device = device
        # engine-wide knobs from the environment (A/B runs of the test suite and the bench), any option:
        # SPARKTS_OPTIONS="hr_grid=1024,fit_pipeline=2"
        for kv in filter(None, os.environ.get("SPARKTS_OPTIONS", "").split(",")):
            name, _, val = kv.partition("=")
            self.set_option(name.strip(), int(val))

    @classmethod
    def get(cls, device=None):
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        with _lock:
            eng = cls._engines.get(device)
        if eng is None:
            eng = Engine(device)
            with _lock:
                cls._engines[device] = eng
        return eng

    def _check(self, rc, what):
        if rc != ARIMA_OK:
            msg = self.L.arima_last_error(self.h)
            raise EngineError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def set_option(self, name, value):
        self._check(self.L.arima_set_option(self.h, name.encode(), int(value)), "arima_set_option")

    def get_option(self, name):
        v = _i64()
        self._check(self.L.arima_get_option(self.h, name.encode(), ctypes.byref(v)), "arima_get_option")
        return int(v.value)

    def synchronize(self):
        """Wait for the device work of every call issued on this handle (the *_device calls are asynchronous)."""
        self._check(self.L.arima_synchronize(self.h), "arima_synchronize")

    def stats(self):
        s = FitStats()
        self._check(self.L.arima_get_last_stats(self.h, ctypes.byref(s)), "arima_get_last_stats")
        return s.as_dict()

    # ---- ARIMA.fitModel over a batch ---------------------------------------------------------------------
    def fit_batch(self, series, p, d, q, include_intercept=True, method="css-cgd", user_init=None):
        series = np.ascontiguousarray(series, dtype=np.float64)
        if series.ndim == 1:
            series = series[None, :]
        N, T = series.shape
        k = p + q + (1 if include_intercept else 0)
        m = METHODS.get(method, 99) if isinstance(method, str) else int(method)
        coef = np.empty((N, max(k, 1)))
        ll = np.empty(N)
        status = np.empty(N, dtype=np.int32)
        n_eval = np.empty(N, dtype=np.int32)
        n_grad = np.empty(N, dtype=np.int32)
        flags = np.empty(N, dtype=np.uint8)
        ui = None
        if user_init is not None:
            ui = np.ascontiguousarray(np.broadcast_to(np.asarray(user_init, dtype=np.float64), (N, k)))
        rc = self.L.arima_fit_batch(self.h, _ptr(series), N, T, p, d, q, int(bool(include_intercept)), m, _ptr(ui),
                                    _ptr(coef), _ptr(ll), _ptr(status, _i32p), _ptr(n_eval, _i32p),
                                    _ptr(n_grad, _i32p), _ptr(flags, _u8p))
        self._check(rc, "arima_fit_batch")
        return dict(coef=coef[:, :k], ll=ll, status=status, n_eval=n_eval, n_grad=n_grad, flags=flags)

    # The *_device methods below wrap asynchronous ABI calls. With blocking=True (the default) they wait for the
    # call's device work before returning, so results can be read through any stream (torch's included); pass
    # blocking=False to keep the ABI's asynchrony and call synchronize() (or stats()) later.
    def fit_batch_device(self, d_series, n_series, T, ld, p, d, q, include_intercept, d_coef, d_ll, d_status,
                         d_n_eval=None, d_n_grad=None, d_flags=None, d_user_init=None, method=METHOD_CSS_CGD,
                         stream=None, blocking=True):
        """Device-pointer entry (ints = raw HBM addresses, e.g. torch tensor .data_ptr())."""
        rc = self.L.arima_fit_batch_device(self.h, d_series, n_series, T, ld, p, d, q, int(bool(include_intercept)),
                                           method, d_user_init, d_coef, d_ll, d_status, d_n_eval, d_n_grad, d_flags,
                                           stream)
        self._check(rc, "arima_fit_batch_device")
        if blocking:
            self.synchronize()

    def sample_device(self, d_series, n_series, T, ld, p, d, q, include_intercept, base_coef, jitter, seed,
                      first_series=0, stream=None, blocking=True):
        base = np.ascontiguousarray(base_coef, dtype=np.float64)
        rc = self.L.arima_sample_batch_device(self.h, d_series, n_series, T, ld, p, d, q, int(bool(include_intercept)),
                                              _ptr(base), float(jitter), int(seed), int(first_series), stream)
        self._check(rc, "arima_sample_batch_device")
        if blocking:
            self.synchronize()

    # ---- building blocks ---------------------------------------------------------------------------------
    def difference(self, series, d):
        series = np.ascontiguousarray(np.atleast_2d(series), dtype=np.float64)
        out = np.empty_like(series)
        self._check(self.L.arima_difference_batch(self.h, _ptr(series), series.shape[0], series.shape[1], d,
                                                  _ptr(out)), "arima_difference_batch")
        return out

    def inverse_difference(self, series, d):
        series = np.ascontiguousarray(np.atleast_2d(series), dtype=np.float64)
        out = np.empty_like(series)
        self._check(self.L.arima_inverse_difference_batch(self.h, _ptr(series), series.shape[0], series.shape[1],
                                                          d, _ptr(out)), "arima_inverse_difference_batch")
        return out

    def css_loglik(self, series, p, d, q, include_intercept, coef):
        series = np.ascontiguousarray(np.atleast_2d(series), dtype=np.float64)
        N, T = series.shape
        k = p + q + (1 if include_intercept else 0)
        coef = np.ascontiguousarray(np.broadcast_to(np.asarray(coef, dtype=np.float64), (N, k)))
        ll = np.empty(N)
        self._check(self.L.arima_css_loglik_batch(self.h, _ptr(series), N, T, p, d, q, int(bool(include_intercept)),
                                                  _ptr(coef), _ptr(ll)), "arima_css_loglik_batch")
        return ll

    def css_gradient(self, diffed, p, q, include_intercept, coef):
        diffed = np.ascontiguousarray(np.atleast_2d(diffed), dtype=np.float64)
        N, n = diffed.shape
        k = p + q + (1 if include_intercept else 0)
        coef = np.ascontiguousarray(np.broadcast_to(np.asarray(coef, dtype=np.float64), (N, k)))
        g = np.empty((N, k))
        self._check(self.L.arima_css_gradient_batch(self.h, _ptr(diffed), N, n, p, q, int(bool(include_intercept)),
                                                    _ptr(coef), _ptr(g)), "arima_css_gradient_batch")
        return g

    def hannan_rissanen(self, diffed, p, q, include_intercept):
        diffed = np.ascontiguousarray(np.atleast_2d(diffed), dtype=np.float64)
        N, n = diffed.shape
        k = p + q + (1 if include_intercept else 0)
        out = np.empty((N, max(k, 1)))
        st = np.empty(N, dtype=np.int32)
        self._check(self.L.arima_hannan_rissanen_batch(self.h, _ptr(diffed), N, n, p, q,
                                                       int(bool(include_intercept)), _ptr(out), _ptr(st, _i32p)),
                    "arima_hannan_rissanen_batch")
        return out[:, :k], st

    def forecast(self, series, p, d, q, include_intercept, coef, n_future):
        series = np.ascontiguousarray(np.atleast_2d(series), dtype=np.float64)
        N, T = series.shape
        k = p + q + (1 if include_intercept else 0)
        coef = np.ascontiguousarray(np.broadcast_to(np.asarray(coef, dtype=np.float64), (N, k)))
        out = np.empty((N, T + n_future))
        self._check(self.L.arima_forecast_batch(self.h, _ptr(series), N, T, p, d, q, int(bool(include_intercept)),
                                                _ptr(coef), n_future, _ptr(out)), "arima_forecast_batch")
        return out

    def forecast_device(self, d_series, n_series, T, ld, p, d, q, include_intercept, d_coef, n_future, d_out, ld_out,
                        stream=None, blocking=True):
        """Device-pointer forecast (ints = raw HBM addresses)."""
        self._check(self.L.arima_forecast_batch_device(self.h, d_series, n_series, T, ld, p, d, q,
                                                       int(bool(include_intercept)), d_coef, n_future, d_out, ld_out,
                                                       stream), "arima_forecast_batch_device")
        if blocking:
            self.synchronize()

    # ---- the TimeSeriesModel pair: ARIMAModel.removeTimeDependentEffects / addTimeDependentEffects ------------
    def _effects(self, name, rows, p, d, q, include_intercept, coef, out):
        rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.float64)
        N, T = rows.shape
        k = p + q + (1 if include_intercept else 0)
        coef = np.ascontiguousarray(np.broadcast_to(np.asarray(coef, dtype=np.float64), (N, k)))
        if out is None:
            out = np.empty((N, T))
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous
                  and out.size == N * T):
            raise ValueError("out must be a C-contiguous float64 array of the input's size")
        self._check(getattr(self.L, name)(self.h, _ptr(rows), N, T, p, d, q, int(bool(include_intercept)),
                                          _ptr(coef), _ptr(out)), name)
        return out

    def remove_effects(self, series, p, d, q, include_intercept, coef, out=None):
        """Residuals of every row under its model (ARIMA.scala:629-644); coef (k,) or (N, k). `out` (optional):
        filled and returned; it may be `series` itself."""
        return self._effects("arima_remove_effects_batch", series, p, d, q, include_intercept, coef, out)

    def add_effects(self, noise, p, d, q, include_intercept, coef, out=None):
        """Every row's model driven by the caller's innovations (ARIMA.scala:655-667)."""
        return self._effects("arima_add_effects_batch", noise, p, d, q, include_intercept, coef, out)

    def remove_effects_device(self, d_series, n_series, T, ld, p, d, q, include_intercept, d_coef, d_out, ld_out,
                              stream=None, blocking=True):
        """Device-pointer residuals (ints = raw HBM addresses); d_out may be d_series with ld_out == ld."""
        self._check(self.L.arima_remove_effects_batch_device(self.h, d_series, n_series, T, ld, p, d, q,
                                                             int(bool(include_intercept)), d_coef, d_out, ld_out,
                                                             stream), "arima_remove_effects_batch_device")
        if blocking:
            self.synchronize()

    def add_effects_device(self, d_noise, n_series, T, ld, p, d, q, include_intercept, d_coef, d_out, ld_out,
                           stream=None, blocking=True):
        """Device-pointer model application; d_out may be d_noise with ld_out == ld."""
        self._check(self.L.arima_add_effects_batch_device(self.h, d_noise, n_series, T, ld, p, d, q,
                                                          int(bool(include_intercept)), d_coef, d_out, ld_out,
                                                          stream), "arima_add_effects_batch_device")
        if blocking:
            self.synchronize()

    # ---- the small models: EWMA (EWMA.scala) and GARCH(1,1) (GARCH.scala) -------------------------------------
    @staticmethod
    def _rows(series):
        series = np.ascontiguousarray(series, dtype=np.float64)
        return series[None, :] if series.ndim == 1 else series

    def _model_fit(self, model, series):
        series = self._rows(series)
        N, T = series.shape
        K = MODEL_PARAMS[model]
        r = dict(coef=np.empty((N, K)), obj=np.empty(N), status=np.empty(N, dtype=np.int32),
                 n_eval=np.empty(N, dtype=np.int32), n_grad=np.empty(N, dtype=np.int32))
        name = f"arima_{model}_fit_batch"
        self._check(getattr(self.L, name)(self.h, _ptr(series), N, T, _ptr(r["coef"]), _ptr(r["obj"]),
                                          _ptr(r["status"], _i32p), _ptr(r["n_eval"], _i32p),
                                          _ptr(r["n_grad"], _i32p)), name)
        return r

    def ewma_fit_batch(self, series):
        """EWMA.fitModel of every row (EWMA.scala:45-69): dict(smoothing N, sse N, status, n_eval, n_grad)."""
        r = self._model_fit("ewma", series)
        return dict(smoothing=r["coef"][:, 0], sse=r["obj"], status=r["status"], n_eval=r["n_eval"],
                    n_grad=r["n_grad"])

    def garch_fit_batch(self, series):
        """GARCH.fitModel of every row (GARCH.scala:33-53): dict(coef N x 3 (omega, alpha, beta), ll N, status, n_eval,
        n_grad)."""
        r = self._model_fit("garch", series)
        return dict(coef=r["coef"], ll=r["obj"], status=r["status"], n_eval=r["n_eval"], n_grad=r["n_grad"])

    def _model_fit_device(self, model, d_series, n_series, T, ld, d_coef, d_obj, d_status, d_n_eval, d_n_grad, stream,
                          blocking):
        name = f"arima_{model}_fit_batch_device"
        self._check(getattr(self.L, name)(self.h, d_series, n_series, T, ld, d_coef, d_obj, d_status, d_n_eval,
                                          d_n_grad, stream), name)
        if blocking:
            self.synchronize()

    def ewma_fit_batch_device(self, d_series, n_series, T, ld, d_smoothing, d_sse, d_status, d_n_eval=None,
                              d_n_grad=None, stream=None, blocking=True):
        """Device-pointer EWMA fits (ints = raw HBM addresses)."""
        self._model_fit_device("ewma", d_series, n_series, T, ld, d_smoothing, d_sse, d_status, d_n_eval, d_n_grad,
                               stream, blocking)

    def garch_fit_batch_device(self, d_series, n_series, T, ld, d_coef, d_ll, d_status, d_n_eval=None, d_n_grad=None,
                               stream=None, blocking=True):
        """Device-pointer GARCH fits; d_coef N x 3 (omega, alpha, beta)."""
        self._model_fit_device("garch", d_series, n_series, T, ld, d_coef, d_ll, d_status, d_n_eval, d_n_grad, stream,
                               blocking)

    def argarch_fit_batch(self, series):
        """ARGARCH.fitModel of every row (GARCH.scala:63-69): dict(coef N x 5 (c, phi, omega, alpha, beta), ll N, status,
        n_eval, n_grad). The AR(1) residuals never exist as a buffer; a row that fails in either stage is all NaN."""
        r = self._model_fit("argarch", series)
        return dict(coef=r["coef"], ll=r["obj"], status=r["status"], n_eval=r["n_eval"], n_grad=r["n_grad"])

    def argarch_fit_batch_device(self, d_series, n_series, T, ld, d_coef, d_ll, d_status, d_n_eval=None,
                                 d_n_grad=None, stream=None, blocking=True):
        """Device-pointer ARGARCH fits; d_coef N x 5 (c, phi, omega, alpha, beta)."""
        self._model_fit_device("argarch", d_series, n_series, T, ld, d_coef, d_ll, d_status, d_n_eval, d_n_grad,
                               stream, blocking)

    def model_fit_stats(self):
        """Round counters of the last EWMA / GARCH / ARGARCH fit (waits for it): n_series, wave_passes, lane_passes,
        max_wave_passes."""
        s = ModelFitStats()
        self._check(self.L.arima_get_last_model_fit_stats(self.h, ctypes.byref(s)), "arima_get_last_model_fit_stats")
        return s.as_dict()

    def _model_call(self, name, model, series, params, out_cols):
        """A building block or an effects call: params (K,) or (N, K), one model per row; out_cols None = N x T."""
        series = self._rows(series)
        N, T = series.shape
        K = MODEL_PARAMS[model]
        params = np.ascontiguousarray(np.broadcast_to(np.asarray(params, dtype=np.float64).reshape(-1, K), (N, K)))
        out = np.empty((N, T) if out_cols is None else (N, out_cols))
        self._check(getattr(self.L, name)(self.h, _ptr(series), N, T, _ptr(params), _ptr(out)), name)
        return out

    def ewma_sse(self, series, smoothing):
        """EWMAModel.sse (EWMA.scala:81-96) of every row under its smoothing: (N,)."""
        return self._model_call("arima_ewma_sse_batch", "ewma", series, smoothing, 1)[:, 0]

    def ewma_gradient(self, series, smoothing):
        """EWMAModel.gradient (EWMA.scala:102-123), the reference's 2 * dJda: (N,)."""
        return self._model_call("arima_ewma_gradient_batch", "ewma", series, smoothing, 1)[:, 0]

    def garch_loglik(self, series, coef):
        """GARCHModel.logLikelihood (GARCH.scala:82-88); coef (3,) or (N, 3) = (omega, alpha, beta): (N,)."""
        return self._model_call("arima_garch_loglik_batch", "garch", series, coef, 1)[:, 0]

    def garch_gradient(self, series, coef):
        """GARCHModel.gradient (GARCH.scala:96-115) in the order it returns, (alpha, beta, omega) halves: (N, 3)."""
        return self._model_call("arima_garch_gradient_batch", "garch", series, coef, 3)

    def ewma_remove_effects(self, series, smoothing):
        """EWMAModel.removeTimeDependentEffects (EWMA.scala:125-133) of every row: (N, T)."""
        return self._model_call("arima_ewma_remove_effects_batch", "ewma", series, smoothing, None)

    def ewma_add_effects(self, series, smoothing):
        """EWMAModel.addTimeDependentEffects (EWMA.scala:135-143), the smoothing recursion: (N, T)."""
        return self._model_call("arima_ewma_add_effects_batch", "ewma", series, smoothing, None)

    def garch_remove_effects(self, series, coef):
        """GARCHModel.removeTimeDependentEffects (GARCH.scala:131-145): the standardised series, (N, T)."""
        return self._model_call("arima_garch_remove_effects_batch", "garch", series, coef, None)

    def garch_add_effects(self, series, coef):
        """GARCHModel.addTimeDependentEffects (GARCH.scala:147-162): the model driven by the rows, (N, T)."""
        return self._model_call("arima_garch_add_effects_batch", "garch", series, coef, None)

    def argarch_remove_effects(self, series, coef):
        """ARGARCHModel.removeTimeDependentEffects (GARCH.scala:205-219); coef (5,) or (N, 5): (N, T)."""
        return self._model_call("arima_argarch_remove_effects_batch", "argarch", series, coef, None)

    def argarch_add_effects(self, series, coef):
        """ARGARCHModel.addTimeDependentEffects (GARCH.scala:221-236), the recursion on dest(i - 1): (N, T)."""
        return self._model_call("arima_argarch_add_effects_batch", "argarch", series, coef, None)

    def garch_sample(self, z, coef):
        """GARCHModel.sample (GARCH.scala:164-185) per row of standard normals z (row i, column t = the t-th
        nextGaussian()); coef (3,) or (N, 3): (N, T) with column 0 equal to 0.0, as in the reference."""
        return self._model_call("arima_garch_sample_batch", "garch", z, coef, None)

    def argarch_sample(self, z, coef):
        """ARGARCHModel.sample (GARCH.scala:238-259) per row of standard normals z; coef (5,) or (N, 5): (N, T)."""
        return self._model_call("arima_argarch_sample_batch", "argarch", z, coef, None)

    def _ar_effects(self, direction, series, p, coef):
        series = self._rows(series)
        N, T = series.shape
        coef = np.ascontiguousarray(np.broadcast_to(np.asarray(coef, dtype=np.float64).reshape(-1, 1 + p), (N, 1 + p)))
        out = np.empty((N, T))
        name = f"arima_ar_{direction}_effects_batch"
        self._check(getattr(self.L, name)(self.h, _ptr(series), N, T, p, _ptr(coef), _ptr(out)), name)
        return out

    def ar_remove_effects(self, series, p, coef):
        """ARModel.removeTimeDependentEffects (Autoregression.scala:60-75) at order p; coef (1 + p,) or (N, 1 + p) =
        (c, phi_1 .. phi_p): (N, T)."""
        return self._ar_effects("remove", series, p, coef)

    def ar_add_effects(self, series, p, coef):
        """ARModel.addTimeDependentEffects (Autoregression.scala:77-90), the recursion on dest: (N, T). With rows of
        standard normals this is ARModel.sample."""
        return self._ar_effects("add", series, p, coef)

    def ar_effects_device(self, direction, d_series, n_series, T, ld, p, d_coef, d_out, ld_out, stream=None,
                          blocking=True):
        """Device-pointer ARModel pair, direction "remove" / "add"; d_coef N x (1 + p); no overlap."""
        name = f"arima_ar_{direction}_effects_batch_device"
        self._check(getattr(self.L, name)(self.h, d_series, n_series, T, ld, p, d_coef, d_out, ld_out, stream), name)
        if blocking:
            self.synchronize()

    def model_sample_device(self, model, d_z, n_series, T, ld, d_coef, d_out, ld_out, stream=None, blocking=True):
        """Device-pointer sample of model "garch" / "argarch" from the normals at d_z; no overlap."""
        name = f"arima_{model}_sample_batch_device"
        self._check(getattr(self.L, name)(self.h, d_z, n_series, T, ld, d_coef, d_out, ld_out, stream), name)
        if blocking:
            self.synchronize()

    def model_effects_device(self, model, direction, d_series, n_series, T, ld, d_params, d_out, ld_out, stream=None,
                             blocking=True):
        """Device-pointer TimeSeriesModel pair of model "ewma" / "garch" / "argarch", direction "remove" / "add" (ints = raw HBM
        addresses; d_params N x K; d_out may not overlap d_series)."""
        name = f"arima_{model}_{direction}_effects_batch_device"
        self._check(getattr(self.L, name)(self.h, d_series, n_series, T, ld, d_params, d_out, ld_out, stream), name)
        if blocking:
            self.synchronize()

    # ---- residual diagnostics: autocorr, dwtest, lbtest per row ---------------------------------------------
    DIAG_OUTPUTS = ("acf", "dw", "lb_stat", "lb_pvalue")

    @staticmethod
    def _diag_bufs(N, max_lag, outputs):
        unknown = set(outputs) - set(Engine.DIAG_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown diagnostics outputs {sorted(unknown)}")
        return {name: (np.empty((N, max_lag) if name == "acf" else (N,)) if name in outputs else None)
                for name in Engine.DIAG_OUTPUTS}

    def diagnostics(self, rows, max_lag, outputs=DIAG_OUTPUTS):
        """autocorr lags 1..max_lag (N, max_lag), dwtest (N,), lbtest statistic and p-value (N,) of every row
        (UnivariateTimeSeries.scala:70-96, TimeSeriesStatisticalTests.scala:251-262, :298-307): a dict of the
        requested `outputs`. With only "dw" requested, max_lag is ignored."""
        rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.float64)
        N, T = rows.shape
        o = self._diag_bufs(N, max_lag, outputs)
        self._check(self.L.arima_diagnostics_batch(self.h, _ptr(rows), N, T, max_lag, _ptr(o["acf"]), _ptr(o["dw"]),
                                                   _ptr(o["lb_stat"]), _ptr(o["lb_pvalue"])),
                    "arima_diagnostics_batch")
        return {k: v for k, v in o.items() if v is not None}

    def residual_diagnostics(self, series, p, d, q, include_intercept, coef, max_lag, outputs=DIAG_OUTPUTS):
        """`diagnostics` of the residuals of every series under its model (removeTimeDependentEffects,
        ARIMA.scala:629-644), computed on the device slice by slice: the residuals never reach the host."""
        series = np.ascontiguousarray(np.atleast_2d(series), dtype=np.float64)
        N, T = series.shape
        k = p + q + (1 if include_intercept else 0)
        coef = np.ascontiguousarray(np.broadcast_to(np.asarray(coef, dtype=np.float64), (N, k)))
        o = self._diag_bufs(N, max_lag, outputs)
        self._check(self.L.arima_residual_diagnostics_batch(self.h, _ptr(series), N, T, p, d, q,
                                                            int(bool(include_intercept)), _ptr(coef), max_lag,
                                                            _ptr(o["acf"]), _ptr(o["dw"]), _ptr(o["lb_stat"]),
                                                            _ptr(o["lb_pvalue"])),
                    "arima_residual_diagnostics_batch")
        return {k_: v for k_, v in o.items() if v is not None}

    def diagnostics_device(self, d_rows, n_series, T, ld, max_lag, d_acf=None, d_dw=None, d_lb_stat=None,
                           d_lb_pvalue=None, stream=None, blocking=True):
        """Device-pointer diagnostics (ints = raw HBM addresses; None = output not wanted)."""
        self._check(self.L.arima_diagnostics_batch_device(self.h, d_rows, n_series, T, ld, max_lag, d_acf, d_dw,
                                                          d_lb_stat, d_lb_pvalue, stream),
                    "arima_diagnostics_batch_device")
        if blocking:
            self.synchronize()

    def residual_diagnostics_device(self, d_series, n_series, T, ld, p, d, q, include_intercept, d_coef, max_lag,
                                    d_acf=None, d_dw=None, d_lb_stat=None, d_lb_pvalue=None, stream=None,
                                    blocking=True):
        """Device-pointer diagnostics of the residuals under the models in d_coef (N x k)."""
        self._check(self.L.arima_residual_diagnostics_batch_device(self.h, d_series, n_series, T, ld, p, d, q,
                                                                   int(bool(include_intercept)), d_coef, max_lag,
                                                                   d_acf, d_dw, d_lb_stat, d_lb_pvalue, stream),
                    "arima_residual_diagnostics_batch_device")
        if blocking:
            self.synchronize()

    # ---- regressions over a regressor matrix: AutoregressionX, bgtest, bptest --------------------------------
    @staticmethod
    def _xreg(x, N, T):
        """The reference's regressor matrix in the ABI's layout: x (T, k) is one matrix shared by every series, x
        (N, T, k) one per series; None: no regressors. Returns (k rows of T values per series, x_series_stride, k)."""
        if x is None:
            return None, 0, 0
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x[:, None]
        if x.ndim == 2 and x.shape[0] == T:
            return np.ascontiguousarray(x.T), 0, x.shape[1]
        if x.ndim == 3 and x.shape[:2] == (N, T):
            return np.ascontiguousarray(x.transpose(0, 2, 1)), x.shape[2] * T, x.shape[2]
        raise ValueError(f"x must be (T, k) or (N, T, k) with N = {N}, T = {T}; got {x.shape}")

    def arx_num_coef(self, n_xcols, y_max_lag, x_max_lag, include_original_x=True):
        K = self.L.arima_arx_num_coef(n_xcols, y_max_lag, x_max_lag, int(bool(include_original_x)))
        if K < 0:
            raise EngineError("arima_arx_num_coef: negative lag or column count")
        return K

    def arx_fit(self, series, x, y_max_lag, x_max_lag, include_original_x=True, no_intercept=False):
        """AutoregressionX.fitModel of every row (AutoregressionX.scala:48-92); x (T, k) shared or (N, T, k):
        dict(coef N x (1 + K) = (c, coefficients), status N)."""
        series = self._rows(series)
        N, T = series.shape
        xr, xs, k = self._xreg(x, N, T)
        K = self.arx_num_coef(k, y_max_lag, x_max_lag, include_original_x)
        coef = np.empty((N, 1 + K))
        status = np.empty(N, dtype=np.int32)
        self._check(self.L.arima_arx_fit_batch(self.h, _ptr(series), N, T, _ptr(xr), xs, k, y_max_lag, x_max_lag,
                                               int(bool(include_original_x)), int(bool(no_intercept)), _ptr(coef),
                                               _ptr(status, _i32p)), "arima_arx_fit_batch")
        return dict(coef=coef, status=status)

    def arx_predict(self, series, x, y_max_lag, x_max_lag, include_original_x, coef):
        """ARXModel.predict of every row (:117-130); coef (1 + K,) or (N, 1 + K) = (c, coefficients):
        (N, T - max(y_max_lag, x_max_lag))."""
        series = self._rows(series)
        N, T = series.shape
        xr, xs, k = self._xreg(x, N, T)
        K = self.arx_num_coef(k, y_max_lag, x_max_lag, include_original_x)
        coef = np.ascontiguousarray(np.broadcast_to(np.asarray(coef, dtype=np.float64).reshape(-1, 1 + K), (N, 1 + K)))
        out = np.empty((N, max(T - max(y_max_lag, x_max_lag), 0)))
        self._check(self.L.arima_arx_predict_batch(self.h, _ptr(series), N, T, _ptr(xr), xs, k, y_max_lag, x_max_lag,
                                                   int(bool(include_original_x)), _ptr(coef), _ptr(out)),
                    "arima_arx_predict_batch")
        return out

    def _regress_test(self, name, residuals, factors, *lag):
        residuals = self._rows(residuals)
        N, T = residuals.shape
        xr, xs, k = self._xreg(factors, N, T)
        r = dict(stat=np.empty(N), pvalue=np.empty(N), status=np.empty(N, dtype=np.int32))
        self._check(getattr(self.L, name)(self.h, _ptr(residuals), N, T, _ptr(xr), xs, k, *lag, _ptr(r["stat"]),
                                          _ptr(r["pvalue"]), _ptr(r["status"], _i32p)), name)
        return r

    def bgtest(self, residuals, factors, max_lag):
        """TimeSeriesStatisticalTests.bgtest (TimeSeriesStatisticalTests.scala:276-288) of every row; factors (T, k)
        shared or (N, T, k): dict(stat N, pvalue N, status N)."""
        return self._regress_test("arima_bgtest_batch", residuals, factors, int(max_lag))

    def bptest(self, residuals, factors):
        """TimeSeriesStatisticalTests.bptest (:320-329) of every row: dict(stat N, pvalue N, status N)."""
        return self._regress_test("arima_bptest_batch", residuals, factors)

    def regarima_co_fit(self, series, x, max_iter=10):
        """RegressionARIMA.fitCochraneOrcutt of every row (RegressionARIMA.scala:83-160); x (T, k) shared or (N, T, k):
        dict(coef N x (1 + k) = regressionCoeff, rho N = arimaCoeff(0), n_iter N, status N)."""
        series = self._rows(series)
        N, T = series.shape
        xr, xs, k = self._xreg(x, N, T)
        r = dict(coef=np.empty((N, 1 + k)), rho=np.empty(N), n_iter=np.empty(N, dtype=np.int32),
                 status=np.empty(N, dtype=np.int32))
        self._check(self.L.arima_regarima_co_fit_batch(self.h, _ptr(series), N, T, _ptr(xr), xs, k, int(max_iter),
                                                       _ptr(r["coef"]), _ptr(r["rho"]), _ptr(r["n_iter"], _i32p),
                                                       _ptr(r["status"], _i32p)), "arima_regarima_co_fit_batch")
        return r

    def arx_fit_device(self, d_series, n_series, T, ld, d_xreg, x_series_stride, n_xcols, y_max_lag, x_max_lag,
                       include_original_x, no_intercept, d_coef, d_status, stream=None, blocking=True):
        """Device-pointer AutoregressionX fits (ints = raw HBM addresses); d_xreg per series n_xcols rows of T values,
        x_series_stride 0 = shared; d_coef N x (1 + K)."""
        self._check(self.L.arima_arx_fit_batch_device(self.h, d_series, n_series, T, ld, d_xreg, x_series_stride,
                                                      n_xcols, y_max_lag, x_max_lag, int(bool(include_original_x)),
                                                      int(bool(no_intercept)), d_coef, d_status, stream),
                    "arima_arx_fit_batch_device")
        if blocking:
            self.synchronize()

    def arx_predict_device(self, d_series, n_series, T, ld, d_xreg, x_series_stride, n_xcols, y_max_lag, x_max_lag,
                           include_original_x, d_coef, d_out, ld_out, stream=None, blocking=True):
        """Device-pointer ARXModel.predict; d_out N x (T - maxLag) with row stride ld_out."""
        self._check(self.L.arima_arx_predict_batch_device(self.h, d_series, n_series, T, ld, d_xreg, x_series_stride,
                                                          n_xcols, y_max_lag, x_max_lag,
                                                          int(bool(include_original_x)), d_coef, d_out, ld_out, stream),
                    "arima_arx_predict_batch_device")
        if blocking:
            self.synchronize()

    def bgtest_device(self, d_residuals, n_series, T, ld, d_factors, x_series_stride, n_xcols, max_lag, d_stat,
                      d_pvalue, d_status, stream=None, blocking=True):
        """Device-pointer bgtest (ints = raw HBM addresses)."""
        self._check(self.L.arima_bgtest_batch_device(self.h, d_residuals, n_series, T, ld, d_factors, x_series_stride,
                                                     n_xcols, max_lag, d_stat, d_pvalue, d_status, stream),
                    "arima_bgtest_batch_device")
        if blocking:
            self.synchronize()

    def bptest_device(self, d_residuals, n_series, T, ld, d_factors, x_series_stride, n_xcols, d_stat, d_pvalue,
                      d_status, stream=None, blocking=True):
        """Device-pointer bptest (ints = raw HBM addresses)."""
        self._check(self.L.arima_bptest_batch_device(self.h, d_residuals, n_series, T, ld, d_factors, x_series_stride,
                                                     n_xcols, d_stat, d_pvalue, d_status, stream),
                    "arima_bptest_batch_device")
        if blocking:
            self.synchronize()

    def regarima_co_fit_device(self, d_series, n_series, T, ld, d_xreg, x_series_stride, n_xcols, max_iter, d_coef,
                               d_rho, d_n_iter, d_status, stream=None, blocking=True):
        """Device-pointer Cochrane-Orcutt fits (ints = raw HBM addresses); d_coef N x (1 + n_xcols), d_n_iter may be
        None."""
        self._check(self.L.arima_regarima_co_fit_batch_device(self.h, d_series, n_series, T, ld, d_xreg,
                                                              x_series_stride, n_xcols, int(max_iter), d_coef, d_rho,
                                                              d_n_iter, d_status, stream),
                    "arima_regarima_co_fit_batch_device")
        if blocking:
            self.synchronize()

    # ---- ARIMAX.fitModel / ARIMAXModel.forecast over a batch (ARIMAX.scala) ----------------------------------
    def arimax_num_coef(self, n_xcols, p, q, xreg_max_lag, include_original_xreg=True):
        K = self.L.arima_arimax_num_coef(n_xcols, p, q, xreg_max_lag, int(bool(include_original_xreg)))
        if K < 0:
            raise EngineError("arima_arimax_num_coef: negative order, lag or column count")
        return K

    def arimax_fit(self, series, x, p, d, q, xreg_max_lag, include_original_xreg=True, include_intercept=True,
                   user_init=None):
        """ARIMAX.fitModel of every row (ARIMAX.scala:59-87); x (T, k) shared or (N, T, k); user_init (K',) or
        (N, K'): dict(coef N x K', ll, status, n_eval, n_grad)."""
        series = self._rows(series)
        N, T = series.shape
        xr, xs, k = self._xreg(x, N, T)
        K = self.arimax_num_coef(k, p, q, xreg_max_lag, include_original_xreg)
        ui = None
        if user_init is not None:
            ui = np.ascontiguousarray(np.broadcast_to(np.asarray(user_init, dtype=np.float64).reshape(-1, K), (N, K)))
        r = dict(coef=np.empty((N, K)), ll=np.empty(N), status=np.empty(N, dtype=np.int32),
                 n_eval=np.empty(N, dtype=np.int32), n_grad=np.empty(N, dtype=np.int32))
        self._check(self.L.arima_arimax_fit_batch(self.h, _ptr(series), N, T, _ptr(xr), xs, k, p, d, q, xreg_max_lag,
                                                  int(bool(include_original_xreg)), int(bool(include_intercept)),
                                                  _ptr(ui), _ptr(r["coef"]), _ptr(r["ll"]), _ptr(r["status"], _i32p),
                                                  _ptr(r["n_eval"], _i32p), _ptr(r["n_grad"], _i32p)),
                    "arima_arimax_fit_batch")
        return r

    def arimax_forecast(self, series, x, p, d, q, xreg_max_lag, include_original_xreg, include_intercept, coef):
        """ARIMAXModel.forecast of every row (:201-256); x (nFuture, k) shared or (N, nFuture, k); coef (K',) or
        (N, K'): (N, T), the last T of the T + nFuture values."""
        series = self._rows(series)
        N, T = series.shape
        x = np.asarray(x, dtype=np.float64)
        if x.ndim not in (2, 3) or (x.ndim == 3 and x.shape[0] != N):
            raise ValueError(f"x must be (nFuture, k) or (N, nFuture, k) with N = {N}; got {x.shape}")
        n_future, k = x.shape[-2], x.shape[-1]
        xr = np.ascontiguousarray(np.swapaxes(x, -1, -2))
        xs = 0 if x.ndim == 2 else k * n_future
        K = self.arimax_num_coef(k, p, q, xreg_max_lag, include_original_xreg)
        coef = np.ascontiguousarray(np.broadcast_to(np.asarray(coef, dtype=np.float64).reshape(-1, K), (N, K)))
        out = np.empty((N, T))
        self._check(self.L.arima_arimax_forecast_batch(self.h, _ptr(series), N, T, _ptr(xr), xs, k, n_future, p, d, q,
                                                       xreg_max_lag, int(bool(include_original_xreg)),
                                                       int(bool(include_intercept)), _ptr(coef), _ptr(out)),
                    "arima_arimax_forecast_batch")
        return out

    def arimax_fit_device(self, d_series, n_series, T, ld, d_xreg, x_series_stride, n_xcols, p, d, q, xreg_max_lag,
                          include_original_xreg, include_intercept, d_coef, d_ll, d_status, d_n_eval=None,
                          d_n_grad=None, d_user_init=None, stream=None, blocking=True):
        """Device-pointer ARIMAX fits (ints = raw HBM addresses); d_xreg per series n_xcols rows of T values,
        x_series_stride 0 = shared; d_coef N x K'."""
        self._check(self.L.arima_arimax_fit_batch_device(self.h, d_series, n_series, T, ld, d_xreg, x_series_stride,
                                                         n_xcols, p, d, q, xreg_max_lag,
                                                         int(bool(include_original_xreg)),
                                                         int(bool(include_intercept)), d_user_init, d_coef, d_ll,
                                                         d_status, d_n_eval, d_n_grad, stream),
                    "arima_arimax_fit_batch_device")
        if blocking:
            self.synchronize()

    def arimax_forecast_device(self, d_series, n_series, T, ld, d_xreg, x_series_stride, n_xcols, n_future, p, d, q,
                               xreg_max_lag, include_original_xreg, include_intercept, d_coef, d_out, ld_out,
                               stream=None, blocking=True):
        """Device-pointer ARIMAXModel.forecast; d_xreg per series n_xcols rows of n_future values; d_out N x T with row
        stride ld_out."""
        self._check(self.L.arima_arimax_forecast_batch_device(self.h, d_series, n_series, T, ld, d_xreg,
                                                              x_series_stride, n_xcols, n_future, p, d, q,
                                                              xreg_max_lag, int(bool(include_original_xreg)),
                                                              int(bool(include_intercept)), d_coef, d_out, ld_out,
                                                              stream),
                    "arima_arimax_forecast_batch_device")
        if blocking:
            self.synchronize()

    def order_search_device(self, d_series, n_series, T, ld, max_p, max_d, max_q, intercept_mode, d_order, d_coef,
                            d_aic, method=METHOD_CSS_CGD, stream=None, blocking=True):
        """Device-pointer order search (ints = raw HBM addresses)."""
        self._check(self.L.arima_order_search_batch_device(self.h, d_series, n_series, T, ld, max_p, max_d, max_q,
                                                           intercept_mode, method, d_order, d_coef, d_aic, stream),
                    "arima_order_search_batch_device")
        if blocking:
            self.synchronize()

    def order_search(self, series, max_p=5, max_d=2, max_q=5, intercept_mode=2, method=METHOD_CSS_CGD):
        """Min-approxAIC model over the (d, p, q, intercept) grid per series (see include/sparkts_arima.h).
        Returns order (N x 4: p, d, q, intercept; -1 when nothing qualified), coef (N x 11), aic (N)."""
        series = np.ascontiguousarray(np.atleast_2d(series), dtype=np.float64)
        N, T = series.shape
        order = np.empty((N, 4), dtype=np.int32)
        coef = np.empty((N, 11))
        aic = np.empty(N)
        self._check(self.L.arima_order_search_batch(self.h, _ptr(series), N, T, max_p, max_d, max_q, intercept_mode,
                                                    method, _ptr(order, _i32p), _ptr(coef), _ptr(aic)),
                    "arima_order_search_batch")
        return order, coef, aic

    def autofit(self, series, max_p=5, max_d=2, max_q=5):
        """ARIMA.autoFit per series (see include/sparkts_arima.h). Returns dict(order N x 4 (p, d, q, intercept),
        coef N x 11, aic N, status N, n_fits N)."""
        series = np.ascontiguousarray(np.atleast_2d(series), dtype=np.float64)
        N, T = series.shape
        out = dict(order=np.empty((N, 4), dtype=np.int32), coef=np.empty((N, 11)), aic=np.empty(N),
                   status=np.empty(N, dtype=np.int32), n_fits=np.empty(N, dtype=np.int32))
        self._check(self.L.arima_autofit_batch(self.h, _ptr(series), N, T, max_p, max_d, max_q,
                                               _ptr(out["order"], _i32p), _ptr(out["coef"]), _ptr(out["aic"]),
                                               _ptr(out["status"], _i32p), _ptr(out["n_fits"], _i32p)),
                    "arima_autofit_batch")
        return out

    def autofit_device(self, d_series, n_series, T, ld, max_p, max_d, max_q, d_order, d_coef, d_aic, d_status,
                       d_n_fits=None, stream=None, blocking=True):
        """Device-pointer autoFit (ints = raw HBM addresses)."""
        self._check(self.L.arima_autofit_batch_device(self.h, d_series, n_series, T, ld, max_p, max_d, max_q, d_order,
                                                      d_coef, d_aic, d_status, d_n_fits, stream),
                    "arima_autofit_batch_device")
        if blocking:
            self.synchronize()

    def kpss(self, series):
        """TimeSeriesStatisticalTests.kpsstest(ts, "c") per series: (stat N, status N)."""
        series = np.ascontiguousarray(np.atleast_2d(series), dtype=np.float64)
        N, T = series.shape
        stat = np.empty(N)
        st = np.empty(N, dtype=np.int32)
        self._check(self.L.arima_kpss_batch(self.h, _ptr(series), N, T, _ptr(stat), _ptr(st, _i32p)),
                    "arima_kpss_batch")
        return stat, st

    def model_flags(self, coef, p, q, include_intercept):
        k = p + q + (1 if include_intercept else 0)
        coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float64).reshape(-1, max(k, 1))[:, :k])
        N = coef.shape[0]
        out = np.empty(N, dtype=np.uint8)
        self._check(self.L.arima_model_flags_batch(self.h, _ptr(coef), N, p, q, int(bool(include_intercept)),
                                                   _ptr(out, _u8p)), "arima_model_flags_batch")
        return out
