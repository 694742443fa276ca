"""The argument contract of every non-fit entry point of the C ABI (include/sparkts_arima.h), as a table: per entry point
the argument faults it refuses, in the order it checks them, with the return code and the arima_last_error text; the
"nothing to do" returns; every output placed on every input and on every other output; and, per host-flavour family,
two valid calls in a row on a fresh handle (3 series, then 5: the staging grows between them) against the reference
the family's own test uses, plus one sequence of calls that stage different sets of arrays back to back.

Shapes: N = 3, T = 12, ARIMA(2,1,2)+c, max_lag 3. Every refused call, and every call with nothing to do, must leave all
of its buffers as they were (inputs and sentinel-filled outputs alike). A check that fails without setting a message
of its own leaves the handle's previous message in place; each row therefore starts from a known one (MARK)."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest

import arimax_ref as AXR
import oracle as O
import regarima_ref as CO
import regress_ref as RR
import smallfit_ref as R
import sparkts_amd._lib as L
from test_gpu_autofit import check_autofit
from test_gpu_diag import _check as diag_check, _p_close, _ref as diag_ref

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED, DEVICE = 0, -1, -2, -3
MARK = "unknown option"                 # what arima_set_option leaves behind for a name it does not know
SENT = 0xA5                             # every byte of every buffer that holds no input
GAP = 256                               # bytes between two buffers of one call
S = NS(N=3, T=12, ld=16, ldo=20, p=2, d=1, q=2, I=1, k=5, nf=4, lag=3)
ROWS_H = S.N * S.T * 8                                   # contiguous host rows
ROWS_D = ((S.N - 1) * S.ld + S.T) * 8                    # strided device rows
OUT_D = ((S.N - 1) * S.ldo + S.T) * 8
ND, NI = S.N * 8, S.N * 4


def B(name, role, nbytes, required=True):
    """A buffer argument: role "in" or "out"; required: a null pointer is refused."""
    return NS(name=name, role=role, nbytes=nbytes, required=required, buf=True)


def V(name, value):
    return NS(name=name, value=value, buf=False)


ORDERS = [V("p", S.p), V("d", S.d), V("q", S.q), V("I", S.I)]
BAD_ORDER = [("p < 0", dict(p=-1), INVALID, "orders"), ("intercept 2", dict(I=2), INVALID, "orders"),
             ("p > 20", dict(p=21), UNSUPPORTED, "orders")]
BAD_D = [("d > 16", dict(d=17, T=20, ld=20, ldo=24), UNSUPPORTED, "orders")]


# The building blocks do not look at their pointers: a null one reaches the copy to or from the device, which refuses it
# (hipErrorInvalidValue) before or after the launch. What such a call wrote before it failed is not pinned, its inputs are.
UNCHECKED = (DEVICE, "invalid argument")


def spec(fn, device, args, faults, null=(INVALID, "null buffer"), overlap=None, n0=(OK, MARK), zero=(), alias_in=None):
    """faults: (label, scalar overrides, rc, message); null: what a null required buffer returns; overlap: the message of a refused overlap (None: the entry point
    does not look), or the pair of messages (an output on an input, an output on another output); n0: what N = 0 with every buffer null returns; zero: overrides of further early-OK calls;
    alias_in: the input an output may alias exactly (the overlap rows shift that output by one element)."""
    return NS(fn=fn, device=device, args=args, faults=faults, null=null, overlap=overlap, n0=n0, zero=zero,
              alias_in=alias_in)


def _effects_specs():
    out = []
    for which in ("remove", "add"):
        out.append(spec(f"arima_{which}_effects_batch", False,
                        [B("rows", "in", ROWS_H), V("N", S.N), V("T", S.T)] + ORDERS +
                        [B("coef", "in", S.N * S.k * 8), B("out", "out", ROWS_H)],
                        BAD_ORDER + BAD_D + [("N < 0", dict(N=-1), INVALID, "bad shape"),
                                             ("T < d", dict(T=0), INVALID, "bad shape")],
                        overlap="out overlaps an input", zero=[dict(T=0, d=0)], alias_in="rows"))
        out.append(spec(f"arima_{which}_effects_batch_device", True,
                        [B("rows", "in", ROWS_D), V("N", S.N), V("T", S.T), V("ld", S.ld)] + ORDERS +
                        [B("coef", "in", S.N * S.k * 8), B("out", "out", OUT_D), V("ldo", S.ldo), V("stream", None)],
                        BAD_ORDER + BAD_D + [("N < 0", dict(N=-1), INVALID, "bad shape"),
                                             ("T < d", dict(T=0), INVALID, "bad shape"),
                                             ("ld < T", dict(ld=S.T - 1), INVALID, "bad shape"),
                                             ("ld_out < T", dict(ldo=S.T - 1), INVALID, "bad shape")],
                        overlap="out overlaps an input", zero=[dict(T=0, d=0)], alias_in="rows"))
    return out


def _diag_specs():
    outs = [B("acf", "out", S.N * S.lag * 8, False), B("dw", "out", ND, False), B("lbs", "out", ND, False),
            B("lbp", "out", ND, False)]
    lags = [("N < 0", dict(N=-1), INVALID, "diagnostics"), ("T < 0", dict(T=-1), INVALID, "diagnostics"),
            ("max_lag 0", dict(lag=0), INVALID, "diagnostics"), ("max_lag T", dict(lag=S.T), INVALID, "diagnostics")]
    # with orders, T < 0 is T < d: refused one check earlier
    lags_resid = [("N < 0", dict(N=-1), INVALID, "diagnostics"), ("T < 0", dict(T=-1, d=0), INVALID, "bad shape")] + lags[2:]
    return [
        spec("arima_diagnostics_batch", False,
             [B("rows", "in", ROWS_H), V("N", S.N), V("T", S.T), V("lag", S.lag)] + outs,
             lags, overlap="overlap", zero=[dict(T=0)]),
        spec("arima_diagnostics_batch_device", True,
             [B("rows", "in", ROWS_D), V("N", S.N), V("T", S.T), V("ld", S.ld), V("lag", S.lag)] + outs +
             [V("stream", None)],
             [("ld < T", dict(ld=S.T - 1), INVALID, "bad shape"),
              ("ld < T before N < 0", dict(ld=S.T - 1, N=-1), INVALID, "bad shape")] + lags,
             overlap="overlap", zero=[dict(T=0)]),
        spec("arima_residual_diagnostics_batch", False,
             [B("rows", "in", ROWS_H), V("N", S.N), V("T", S.T)] + ORDERS +
             [B("coef", "in", S.N * S.k * 8), V("lag", S.lag)] + outs,
             BAD_ORDER + BAD_D + [("T < d", dict(T=0), INVALID, "bad shape")] + lags_resid,
             overlap="overlap", zero=[dict(T=0, d=0)]),
        spec("arima_residual_diagnostics_batch_device", True,
             [B("rows", "in", ROWS_D), V("N", S.N), V("T", S.T), V("ld", S.ld)] + ORDERS +
             [B("coef", "in", S.N * S.k * 8), V("lag", S.lag)] + outs + [V("stream", None)],
             BAD_ORDER + BAD_D + [("T < d", dict(T=0), INVALID, "bad shape"),
                                  ("ld < T", dict(ld=S.T - 1), INVALID, "bad shape")] + lags_resid,
             overlap="overlap", zero=[dict(T=0, d=0)]),
    ]


def _model_specs():
    out = []
    shape1 = [("N < 0", dict(N=-1), INVALID, "bad shape"), ("T < 1", dict(T=0), INVALID, "bad shape")]
    shape0 = [("N < 0", dict(N=-1), INVALID, "bad shape"), ("T < 0", dict(T=-1), INVALID, "bad shape")]
    for m, K in (("ewma", 1), ("garch", 3)):
        fit_outs = [B("coef", "out", ND * K), B("obj", "out", ND), B("status", "out", NI),
                    B("n_eval", "out", NI, False), B("n_grad", "out", NI, False)]
        out.append(spec(f"arima_{m}_fit_batch", False, [B("rows", "in", ROWS_H), V("N", S.N), V("T", S.T)] + fit_outs,
                        shape1, overlap="overlap"))
        out.append(spec(f"arima_{m}_fit_batch_device", True,
                        [B("rows", "in", ROWS_D), V("N", S.N), V("T", S.T), V("ld", S.ld)] + fit_outs +
                        [V("stream", None)],
                        shape1 + [("ld < T", dict(ld=S.T - 1), INVALID, "bad shape")], overlap="overlap"))
        evals = (("sse", 1), ("gradient", 1)) if m == "ewma" else (("loglik", 1), ("gradient", 3))
        for what, cols in evals:
            out.append(spec(f"arima_{m}_{what}_batch", False,
                            [B("rows", "in", ROWS_H), V("N", S.N), V("T", S.T), B("params", "in", ND * K),
                             B("out", "out", ND * cols)], shape1, overlap="overlap"))
        for which in ("remove", "add"):
            out.append(spec(f"arima_{m}_{which}_effects_batch", False,
                            [B("rows", "in", ROWS_H), V("N", S.N), V("T", S.T), B("params", "in", ND * K),
                             B("out", "out", ROWS_H)], shape0, overlap="overlap", zero=[dict(T=0)]))
            out.append(spec(f"arima_{m}_{which}_effects_batch_device", True,
                            [B("rows", "in", ROWS_D), V("N", S.N), V("T", S.T), V("ld", S.ld),
                             B("params", "in", ND * K), B("out", "out", OUT_D), V("ldo", S.ldo), V("stream", None)],
                            shape0 + [("ld < T", dict(ld=S.T - 1), INVALID, "bad shape"),
                                      ("ld_out < T", dict(ldo=S.T - 1), INVALID, "bad shape")],
                            overlap="overlap", zero=[dict(T=0)]))
    return out


# The regressions over a regressor matrix: k = 2 columns, AutoregressionX(yMaxLag 1, xMaxLag 1, includeOriginalX) has
# K = 5 predictors and R = 11 rows, bgtest max_lag 3. The faults in the order regress_check and its callers test them.
RG = NS(k=2, yl=1, xl=1, K=5, R=S.T - 1, xs_h=2 * S.T, xs_d=2 * S.T + 4, ldo=S.T + 2)
RG_OVERLAP = ("an output overlaps an input", "outputs overlap")       # the overlap rule's two messages, passed through


def _regress_specs():
    out = []
    for device in (False, True):
        sfx, xs = ("_device", RG.xs_d) if device else ("", RG.xs_h)
        head = [B("rows", "in", ROWS_D if device else ROWS_H), V("N", S.N), V("T", S.T)] + \
            ([V("ld", S.ld)] if device else []) + \
            [B("xreg", "in", ((S.N - 1) * xs + RG.k * S.T) * 8), V("xs", xs), V("k", RG.k)]
        tail = [V("stream", None)] if device else []
        shape = [("N < 0", dict(N=-1), INVALID, "bad shape"), ("T < 0", dict(T=-1), INVALID, "bad shape")] + \
            ([("ld < T", dict(ld=S.T - 1), INVALID, "bad shape")] if device else []) + \
            [("n_xcols < 0", dict(k=-1), INVALID, "bad shape")]
        stride = [("x_series_stride below n_xcols * T", dict(xs=RG.k * S.T - 1), INVALID,
                   "x_series_stride below n_xcols * T")]
        lags = [("y_max_lag < 0", dict(yl=-1), INVALID, "bad shape"), ("x_max_lag < 0", dict(xl=-1), INVALID, "bad shape")]
        wide = "at most 64 columns"
        arx = [V("yl", RG.yl), V("xl", RG.xl), V("orig", 1)]
        out.append(spec("arima_arx_fit_batch" + sfx, device,
                        head + arx + [V("noint", 0), B("coef", "out", ND * (1 + RG.K)), B("status", "out", NI)] + tail,
                        shape + lags + stride +
                        [("the stride before the columns", dict(xs=RG.k * S.T - 1, yl=62), INVALID, stride[0][3]),
                         ("65 columns", dict(yl=62), UNSUPPORTED, wide),                  # 1 + 62 + 2
                         ("65 columns before N = 0", dict(yl=62, N=0), UNSUPPORTED, wide)],
                        overlap=RG_OVERLAP))
        out.append(spec("arima_arx_predict_batch" + sfx, device,
                        head + arx + [B("coef", "in", ND * (1 + RG.K)),
                                      B("out", "out", ((S.N - 1) * RG.ldo + RG.R) * 8 if device else ND * RG.R)] +
                        ([V("ldo", RG.ldo)] if device else []) + tail,
                        shape + lags + stride +
                        [("65 predictors", dict(yl=61), UNSUPPORTED, wide),               # no ones column: 61 + 2 + 2
                         ("T < maxLag", dict(yl=S.T + 1), INVALID, "bad shape")] +
                        ([("ld_out < R", dict(ldo=RG.R - 1), INVALID, "bad shape")] if device else []),
                        overlap=RG_OVERLAP, zero=[dict(T=1)]))                            # R = 0: nothing to predict
        test_outs = [B("stat", "out", ND), B("pvalue", "out", ND), B("status", "out", NI)]
        out.append(spec("arima_bgtest_batch" + sfx, device, head + [V("lag", S.lag)] + test_outs + tail,
                        shape + [("max_lag < 0", dict(lag=-1), INVALID, "bad shape"),
                                 ("bad shape before max_lag 0", dict(lag=0, N=-1), INVALID, "bad shape"),
                                 ("max_lag 0", dict(lag=0), INVALID, "max_lag < 1"),
                                 ("max_lag 0 before the stride", dict(lag=0, xs=1), INVALID, "max_lag < 1")] + stride +
                        [("65 columns", dict(lag=62), UNSUPPORTED, wide)],                # 1 + 2 + 62
                        overlap=RG_OVERLAP))
        out.append(spec("arima_bptest_batch" + sfx, device, head + test_outs + tail,
                        shape + [("n_xcols 0", dict(k=0), INVALID, "n_xcols < 1")] + stride +
                        [("65 columns", dict(k=64, xs=0), UNSUPPORTED, wide)],            # 1 + 64, one shared matrix
                        overlap=RG_OVERLAP))
    return out


# RegressionARIMA's Cochrane-Orcutt fit over the same k = 2 regressor block: co_check tests max_iter, then n_xcols,
# then regress_check's rules, then its own width (the ones column is always there, so 64 regressors are one too many).
def _regarima_specs():
    out = []
    for device in (False, True):
        sfx, xs = ("_device", RG.xs_d) if device else ("", RG.xs_h)
        args = [B("rows", "in", ROWS_D if device else ROWS_H), V("N", S.N), V("T", S.T)] + \
            ([V("ld", S.ld)] if device else []) + \
            [B("xreg", "in", ((S.N - 1) * xs + RG.k * S.T) * 8), V("xs", xs), V("k", RG.k), V("iters", 5),
             B("coef", "out", ND * (1 + RG.k)), B("rho", "out", ND), B("n_iter", "out", NI, False),
             B("status", "out", NI)] + ([V("stream", None)] if device else [])
        wide = "at most 64 columns"
        out.append(spec("arima_regarima_co_fit_batch" + sfx, device, args,
                        [("max_iter 0", dict(iters=0), INVALID, "max_iter < 1"),
                         ("max_iter before n_xcols", dict(iters=0, k=0), INVALID, "max_iter < 1"),
                         ("n_xcols 0", dict(k=0), INVALID, "n_xcols < 1"),
                         ("n_xcols < 0", dict(k=-1), INVALID, "n_xcols < 1"),
                         ("n_xcols before the shape", dict(k=0, N=-1), INVALID, "n_xcols < 1"),
                         ("N < 0", dict(N=-1), INVALID, "bad shape"), ("T < 0", dict(T=-1), INVALID, "bad shape")] +
                        ([("ld < T", dict(ld=S.T - 1), INVALID, "bad shape")] if device else []) +
                        [("x_series_stride below n_xcols * T", dict(xs=RG.k * S.T - 1), INVALID,
                          "x_series_stride below n_xcols * T"),
                         ("the stride before the columns", dict(xs=1, k=64), INVALID, "x_series_stride below n_xcols * T"),
                         ("65 regressors", dict(k=65, xs=0), UNSUPPORTED, wide),          # regress_check's own count
                         ("64 regressors and the ones column", dict(k=64, xs=0), UNSUPPORTED, wide),
                         ("65 columns at N = 0", dict(k=64, xs=0, N=0), UNSUPPORTED, wide)],
                        overlap=RG_OVERLAP))
    return out


# ARIMAX(1, 1, 1) with xreg_max_lag 1 and the original columns over k = 2 regressors: K' = 1 + 1 + 1 + 2 + 2 = 7
# coefficients; the forecast reads n_future = 4 regressor rows. The faults in the order arimax_check, the device
# forecast's own ld_out test and arimax_forecast_check test them.
AX = NS(p=1, d=1, q=1, L=1, Kp=7, xs_h=RG.k * S.nf, xs_d=RG.k * S.nf + 4)
AX_ORDERS = [V("p", AX.p), V("d", AX.d), V("q", AX.q), V("L", AX.L), V("orig", 1), V("I", 1)]
AX_STRIDE = "x_series_stride below one matrix"


def _arimax_faults(device, forecast):
    """arimax_check's refusals; the rows of a regressor matrix are T for a fit and n_future for a forecast."""
    huge = dict(T=10 ** 9, ld=10 ** 9, ldo=10 ** 9, k=1, xs=0)       # (d + 2) T alone is beyond an int
    return [("N < 0", dict(N=-1), INVALID, "bad shape"), ("T < 0", dict(T=-1), INVALID, "bad shape")] + \
        ([("ld < T", dict(ld=S.T - 1), INVALID, "bad shape")] if device else []) + \
        ([("n_future < 0", dict(nf=-1), INVALID, "bad shape")] if forecast else []) + \
        [("the shape before n_xcols", dict(N=-1, k=0), INVALID, "bad shape"),
         ("n_xcols 0", dict(k=0), INVALID, "n_xcols < 1"),
         ("n_xcols before the orders", dict(k=-1, p=-1), INVALID, "n_xcols < 1"),
         ("p < 0", dict(p=-1), INVALID, "negative order or lag"), ("d < 0", dict(d=-1), INVALID, "negative order or lag"),
         ("q < 0", dict(q=-1), INVALID, "negative order or lag"),
         ("xreg_max_lag < 0", dict(L=-1), INVALID, "negative order or lag"),
         ("the orders before the stride", dict(q=-1, xs=1), INVALID, "negative order or lag"),
         ("x_series_stride below one matrix", dict(xs=RG.k * (S.nf if forecast else S.T) - 1), INVALID, AX_STRIDE),
         ("the stride before p > 20", dict(xs=1, p=21), INVALID, AX_STRIDE),
         ("p > 20", dict(p=21), UNSUPPORTED, "p, q <= 20"), ("q > 20", dict(q=21), UNSUPPORTED, "p, q <= 20"),
         ("p > 20 before d > 16", dict(p=21, d=17), UNSUPPORTED, "p, q <= 20"),
         ("d > 16", dict(d=17), UNSUPPORTED, "d <= 16"),
         ("d > 16 before the coefficients", dict(d=17, L=20, xs=0), UNSUPPORTED, "d <= 16"),
         ("45 coefficients", dict(L=20, xs=0), UNSUPPORTED, "at most 41 coefficients"),      # 3 + 2 * 20 + 2
         ("45 coefficients at N = 0", dict(L=20, xs=0, N=0), UNSUPPORTED, "at most 41 coefficients"),
         ("the regressor matrix beyond an int", dict(k=6 * 10 ** 8, L=0, orig=0, xs=0), UNSUPPORTED,
          "regressor matrix too large")] + \
        ([("the matrix before the series", dict(huge, nf=2 ** 31 - 1, k=2), UNSUPPORTED, "regressor matrix too large")]
         if forecast else []) + \
        [("the series beyond an int", huge, UNSUPPORTED, "series too long")]


def _arimax_specs():
    out = []
    for device in (False, True):
        sfx = "_device" if device else ""
        rows = [B("rows", "in", ROWS_D if device else ROWS_H), V("N", S.N), V("T", S.T)] + \
            ([V("ld", S.ld)] if device else [])
        tail = [V("stream", None)] if device else []
        xs = RG.xs_d if device else RG.xs_h
        out.append(spec("arima_arimax_fit_batch" + sfx, device,
                        rows + [B("xreg", "in", ((S.N - 1) * xs + RG.k * S.T) * 8), V("xs", xs), V("k", RG.k)] +
                        AX_ORDERS + [B("user_init", "in", ND * AX.Kp, False), B("coef", "out", ND * AX.Kp),
                                     B("ll", "out", ND), B("status", "out", NI), B("n_eval", "out", NI, False),
                                     B("n_grad", "out", NI, False)] + tail,
                        _arimax_faults(device, False), overlap=RG_OVERLAP))
        xs = AX.xs_d if device else AX.xs_h
        out.append(spec("arima_arimax_forecast_batch" + sfx, device,
                        rows + [B("xreg", "in", ((S.N - 1) * xs + RG.k * S.nf) * 8), V("xs", xs), V("k", RG.k),
                                V("nf", S.nf)] + AX_ORDERS +
                        [B("coef", "in", ND * AX.Kp), B("out", "out", OUT_D if device else ROWS_H)] +
                        ([V("ldo", S.ldo)] if device else []) + tail,
                        _arimax_faults(device, True) +
                        ([("ld_out < T", dict(ldo=S.T - 1), INVALID, "bad shape"),
                          ("ld_out before the forecast's shapes", dict(ldo=S.T - 1, p=0, q=0), INVALID, "bad shape")]
                         if device else []) +
                        [("p = q = 0", dict(p=0, q=0), INVALID, "max(p, q) == 0"),
                         ("p = q = 0 at N = 0", dict(p=0, q=0, N=0), INVALID, "max(p, q) == 0"),
                         ("p = q = 0 before T < d", dict(p=0, q=0, d=13), INVALID, "max(p, q) == 0"),
                         ("T < d", dict(d=13), INVALID, "T < d"),
                         ("T < d at N = 0", dict(d=13, N=0), INVALID, "T < d"),
                         # R = max(p, q) + max(n_future - d, 0) = 4 differenced regressor rows
                         ("xreg_max_lag above R", dict(L=5), INVALID, "fewer differenced xreg rows than xreg_max_lag"),
                         # R - L = 19 predictor rows, max(p, q) + T - d = 12 of history
                         ("n_future - L above T", dict(nf=20, xs=0), INVALID, "more predictor rows than history")],
                        overlap=RG_OVERLAP,
                        # T = 0 passes the forecast's shapes only with n_future <= xreg_max_lag
                        zero=[dict(T=0, d=0, nf=1)]))
    return out


SEARCH = [V("max_p", 2), V("max_d", 1), V("max_q", 2), V("imode", 2), V("method", 0)]
SEARCH_OUT = [B("order", "out", S.N * 16), B("coef11", "out", S.N * 88), B("aic", "out", ND)]
AUTOFIT_OUT = SEARCH_OUT + [B("status", "out", NI), B("n_fits", "out", NI, False)]
AF_UNSUPPORTED = "autofit: max_p <= 8 (css-bobyqa retries of <= 11 parameters), d <= 16"

SPECS = [
    # the building blocks: a bare code for a bad shape, no null and no overlap checks (the differenced rows of the
    # gradient and of Hannan-Rissanen go through the padded 2-D upload, outside the staging table: no null row for them)
    spec("arima_difference_batch", False, [B("rows", "in", ROWS_H), V("N", S.N), V("T", S.T), V("d", S.d),
                                           B("out", "out", ROWS_H)],
         [("N < 0", dict(N=-1), INVALID, MARK), ("T < 0", dict(T=-1), INVALID, MARK), ("d < 0", dict(d=-1), INVALID, MARK)],
         null=UNCHECKED, zero=[dict(T=0)]),
    spec("arima_inverse_difference_batch", False, [B("rows", "in", ROWS_H), V("N", S.N), V("T", S.T), V("d", S.d),
                                                   B("out", "out", ROWS_H)],
         [("N < 0", dict(N=-1), INVALID, MARK), ("T < 0", dict(T=-1), INVALID, MARK), ("d < 0", dict(d=-1), INVALID, MARK)],
         null=UNCHECKED, zero=[dict(T=0)]),
    spec("arima_css_loglik_batch", False, [B("rows", "in", ROWS_H), V("N", S.N), V("T", S.T)] + ORDERS +
         [B("coef", "in", S.N * S.k * 8), B("ll", "out", ND)],
         BAD_ORDER + BAD_D + [("N < 0", dict(N=-1), INVALID, "bad shape"), ("T < 0", dict(T=-1), INVALID, "bad shape")],
         null=UNCHECKED),
    spec("arima_css_gradient_batch", False, [B("rows", "in", S.N * (S.T - 1) * 8, False), V("N", S.N), V("T", S.T - 1),
                                             V("p", S.p), V("q", S.q), V("I", S.I), B("coef", "in", S.N * S.k * 8),
                                             B("grad", "out", S.N * S.k * 8)],
         BAD_ORDER + [("N < 0", dict(N=-1), INVALID, "bad shape"), ("n < 0", dict(T=-1), INVALID, "bad shape")],
         null=UNCHECKED, zero=[dict(p=0, q=0, I=0)]),
    spec("arima_hannan_rissanen_batch", False, [B("rows", "in", S.N * (S.T - 1) * 8, False), V("N", S.N), V("T", S.T - 1),
                                                V("p", S.p), V("q", S.q), V("I", S.I), B("init", "out", S.N * S.k * 8),
                                                B("status", "out", NI)],
         BAD_ORDER + [("N < 0", dict(N=-1), INVALID, "bad shape"), ("n < 0", dict(T=-1), INVALID, "bad shape")],
         null=UNCHECKED),
    spec("arima_model_flags_batch", False, [B("coef", "in", S.N * S.k * 8), V("N", S.N), V("p", S.p), V("q", S.q),
                                            V("I", S.I), B("flags", "out", S.N)],
         BAD_ORDER, null=UNCHECKED, zero=[dict(N=-1)]),
    spec("arima_kpss_batch", False, [B("rows", "in", ROWS_H), V("N", S.N), V("T", S.T), B("stat", "out", ND),
                                     B("status", "out", NI)],
         [("N < 0", dict(N=-1), INVALID, MARK), ("T < 0", dict(T=-1), INVALID, MARK)]),
    spec("arima_forecast_batch", False, [B("rows", "in", ROWS_H), V("N", S.N), V("T", S.T)] + ORDERS +
         [B("coef", "in", S.N * S.k * 8), V("nf", S.nf), B("out", "out", S.N * (S.T + S.nf) * 8)],
         BAD_ORDER + BAD_D + [("N < 0", dict(N=-1), INVALID, "bad shape"), ("T < d", dict(T=0), INVALID, "bad shape"),
                              ("n_future < 0", dict(nf=-1), INVALID, "bad shape")]),
    spec("arima_forecast_batch_device", True, [B("rows", "in", ROWS_D), V("N", S.N), V("T", S.T), V("ld", S.ld)] +
         ORDERS + [B("coef", "in", S.N * S.k * 8), V("nf", S.nf), B("out", "out", ((S.N - 1) * S.ldo + S.T + S.nf) * 8),
                   V("ldo", S.ldo), V("stream", None)],
         BAD_ORDER + BAD_D + [("N < 0", dict(N=-1), INVALID, "bad shape"), ("T < d", dict(T=0), INVALID, "bad shape"),
                              ("n_future < 0", dict(nf=-1), INVALID, "bad shape"),
                              ("ld < T", dict(ld=S.T - 1), INVALID, "bad shape"),
                              ("ld_out < T + n_future", dict(ldo=S.T + S.nf - 1), INVALID, "bad shape")]),
    spec("arima_sample_batch_device", True, [B("rows", "out", ROWS_D, False), V("N", S.N), V("T", S.T), V("ld", S.ld)] +
         ORDERS + [V("base", "BASE"), V("jitter", 0.05), V("seed", 7), V("first", 0), V("stream", None)],
         [("N < 0", dict(N=-1), INVALID, MARK), ("T < 0", dict(T=-1), INVALID, MARK),
          ("ld < T", dict(ld=S.T - 1), INVALID, MARK), ("null base", dict(base=None), INVALID, MARK)] + BAD_ORDER + BAD_D),
    # the order search checks its bounds and shape inside the shared body, after the host flavour has staged
    spec("arima_order_search_batch", False, [B("rows", "in", ROWS_H), V("N", S.N), V("T", S.T)] + SEARCH + SEARCH_OUT,
         [("N < 0", dict(N=-1), INVALID, "bad shape"), ("T < 0", dict(T=-1), INVALID, "bad shape"),
          ("max_p < 0", dict(max_p=-1), INVALID, "bad search bounds"),
          ("intercept mode 3", dict(imode=3), INVALID, "bad search bounds"),
          ("max_q > 5", dict(max_q=6), UNSUPPORTED, "p, q <= 5, d <= 16")]),
    spec("arima_order_search_batch_device", True,
         [B("rows", "in", ROWS_D, False), V("N", S.N), V("T", S.T), V("ld", S.ld)] + SEARCH + SEARCH_OUT +
         [V("stream", None)],
         [("max_p < 0", dict(max_p=-1), INVALID, "bad search bounds"),
          ("max_d > 16", dict(max_d=17), UNSUPPORTED, "p, q <= 5, d <= 16"),
          ("N < 0", dict(N=-1), INVALID, "bad shape"), ("T < 0", dict(T=-1), INVALID, "bad shape"),
          ("ld < T", dict(ld=S.T - 1), INVALID, "bad shape")],
         null=(INVALID, "bad shape"), n0=(INVALID, "bad shape"), zero=[dict(N=0)]),
    spec("arima_autofit_batch", False, [B("rows", "in", ROWS_H), V("N", S.N), V("T", S.T), V("max_p", 2), V("max_d", 1),
                                        V("max_q", 2)] + AUTOFIT_OUT,
         [("N < 0", dict(N=-1), INVALID, "bad shape"), ("T < 0", dict(T=-1), INVALID, "bad shape"),
          ("max_q < 0", dict(max_q=-1), INVALID, "bad autofit bounds"),
          ("max_p > 8", dict(max_p=9), UNSUPPORTED, AF_UNSUPPORTED)]),
    spec("arima_autofit_batch_device", True, [B("rows", "in", ROWS_D), V("N", S.N), V("T", S.T), V("ld", S.ld),
                                              V("max_p", 2), V("max_d", 1), V("max_q", 2)] + AUTOFIT_OUT +
         [V("stream", None)],
         [("max_q < 0", dict(max_q=-1), INVALID, "bad autofit bounds"),
          ("max_d > 16", dict(max_d=17), UNSUPPORTED, AF_UNSUPPORTED),
          ("N < 0", dict(N=-1), INVALID, "bad shape"), ("T < 0", dict(T=-1), INVALID, "bad shape"),
          ("ld < T", dict(ld=S.T - 1), INVALID, "bad shape")], null=(INVALID, "bad shape")),
] + _effects_specs() + _diag_specs() + _model_specs() + _regress_specs() + _regarima_specs() + _arimax_specs()


def rows_of(sp):
    """The table of one entry point: (label, scalar overrides, pointer placement, rc, message). Placement: a dict
    buffer name -> None (null) or (other buffer's name, byte shift)."""
    bufs = [a for a in sp.args if a.buf]
    ins = [a for a in bufs if a.role == "in"]
    outs = [a for a in bufs if a.role == "out"]
    t = [(label, ov, {}, rc, msg) for label, ov, rc, msg in sp.faults]
    t += [(f"null {a.name}", {}, {a.name: None}, *sp.null) for a in bufs if a.required]
    t.append(("N = 0, every buffer null", dict(N=0), {a.name: None for a in bufs}, *sp.n0))
    t += [(f"early OK {ov}", ov, {}, OK, MARK) for ov in sp.zero]
    if sp.overlap:
        on_in, on_out = sp.overlap if isinstance(sp.overlap, tuple) else (sp.overlap, sp.overlap)
        for i, o in enumerate(outs):
            t += [(f"{o.name} on {a.name}", {}, {o.name: (a.name, 8 if a.name == sp.alias_in else 0)}, INVALID,
                   on_in) for a in ins]
            t += [(f"{o.name} on {o2.name}", {}, {o.name: (o2.name, 0)}, INVALID, on_out) for o2 in outs[i + 1:]]
    if sp.alias_in and sp.device:
        t.append(("out on the rows, another stride", dict(ldo=S.ld + 1), {"out": (sp.alias_in, 0)}, INVALID, sp.overlap))
    return t


class Arena:
    """Every buffer of one call inside one allocation (host: numpy; device: torch), GAP bytes apart, filled with SENT;
    the inputs hold finite doubles. `same()`: nothing in it has changed since it was built."""

    def __init__(self, sp, engine):
        self.off, total = {}, GAP
        for a in sp.args:
            if a.buf:
                self.off[a.name] = total
                total += (a.nbytes + GAP + 255) // 256 * 256
        host = np.full(total, SENT, dtype=np.uint8)
        rng = np.random.default_rng(len(sp.fn))
        for a in sp.args:
            if a.buf and a.role == "in":
                host[self.off[a.name]:self.off[a.name] + a.nbytes] = rng.uniform(0.1, 0.4, a.nbytes // 8).view(np.uint8)
        self.snapshot = host.copy()
        if sp.device:
            import torch
            self.mem = torch.from_numpy(host).to(f"cuda:{engine.device}")
            self.base = self.mem.data_ptr()
        else:
            self.mem = host
            self.base = host.ctypes.data

    def same(self, only=None):
        """only: the buffers to look at (default: every byte)."""
        now = self.mem if isinstance(self.mem, np.ndarray) else self.mem.cpu().numpy()
        if only is None:
            return bool(np.array_equal(now, self.snapshot))
        return all(np.array_equal(now[self.off[a.name]:self.off[a.name] + a.nbytes],
                                  self.snapshot[self.off[a.name]:self.off[a.name] + a.nbytes]) for a in only)

    def reset(self):
        self.mem[:] = self.snapshot


BASE_COEF = np.array([8.2, 0.2, 0.5, 0.3, 0.1])


def call(engine, sp, arena, overrides, placement, handle="h"):
    fn = getattr(engine.L, sp.fn)
    argv = [engine.h if handle == "h" else None]
    for i, a in enumerate(sp.args, start=1):
        if a.buf:
            where = placement.get(a.name, (a.name, 0))
            addr = None if where is None else arena.base + arena.off[where[0]] + where[1]
        else:
            v = overrides.get(a.name, a.value)
            argv.append(L._ptr(BASE_COEF) if isinstance(v, str) else v)
            continue
        typ = fn.argtypes[i]
        argv.append(addr if addr is None or typ is ctypes.c_void_p else ctypes.cast(ctypes.c_void_p(addr), typ))
    return fn(*argv)


def last_error(engine):
    return engine.L.arima_last_error(engine.h).decode()


def mark(engine):
    assert engine.L.arima_set_option(engine.h, b"no such option", 0) == INVALID and last_error(engine) == MARK


def drain(engine):
    """After a call that a HIP copy refused: the runtime keeps that error as its last one until somebody asks for it,
    and the next launch does, so one throw-away launch takes it; the second call must be clean, and being a host-buffer
    call it returns only once the handle's stream has drained."""
    rows, stat, st = np.array([[1.0, 2.0]]), np.zeros(1), np.zeros(1, dtype=np.int32)
    args = (engine.h, L._ptr(rows), 1, 2, L._ptr(stat), L._ptr(st, L._i32p))
    engine.L.arima_kpss_batch(*args)
    assert engine.L.arima_kpss_batch(*args) == OK, last_error(engine)


# ---- 1. refusals and early returns: the code, the message, nothing written ---------------------------------------------
@pytest.mark.parametrize("sp", SPECS, ids=lambda sp: sp.fn)
def test_refusals_and_early_returns(engine, sp):
    arena = Arena(sp, engine)
    mark(engine)
    assert call(engine, sp, arena, {}, {}, handle=None) == INVALID, "null handle"
    assert last_error(engine) == MARK and engine.L.arima_last_error(None) == b"null handle"
    for label, overrides, placement, rc, msg in rows_of(sp):
        mark(engine)
        got = call(engine, sp, arena, overrides, placement)
        assert (got, last_error(engine)) == (rc, msg), f"{sp.fn}: {label}"
        if sp.device:
            engine.synchronize()
        if rc == DEVICE:
            drain(engine)
            assert arena.same([a for a in sp.args if a.buf and a.role == "in"]), f"{sp.fn}: {label}: an input has changed"
            arena.reset()
        assert arena.same(), f"{sp.fn}: {label}: a buffer of the call has changed"


def test_kpss_short_rows_are_answered_on_the_host(engine):
    for T, st in ((0, L.ST_NO_DATA), (1, L.ST_NOT_ENOUGH_DATA)):
        stat, status = engine.kpss(np.zeros((S.N, T)))
        assert np.all(status == st) and np.all(np.isnan(stat))


# ---- 2. valid calls: 3 series, then 5, on a fresh handle; the sequence of different staging tables -------------------
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        return bool(np.all((a.view(np.int64) == np.asarray(b, dtype=np.float64).view(np.int64)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def _data(N):
    rng = np.random.default_rng(20261020)
    s = (np.cumsum(rng.standard_normal((5, S.T)), axis=1) * 3.0 + 5.0)[:N]
    coef = rng.uniform(-0.4, 0.4, (5, S.k))[:N]
    return np.ascontiguousarray(s), np.ascontiguousarray(coef)


def _each(fn, *cols):
    return [fn(*row) for row in zip(*cols)]


def fam_difference(e, N):
    s, _ = _data(N)
    d = e.difference(s, S.d)
    exp = np.stack([O.differences_of_order_d(r, S.d) for r in s])
    assert np.array_equal(d, exp)
    assert np.array_equal(e.inverse_difference(d, S.d), np.stack([O.inverse_differences_of_order_d(r, S.d) for r in exp]))


def fam_css_loglik(e, N):
    s, c = _data(N)
    assert _same(e.css_loglik(s, S.p, S.d, S.q, True, c), _each(lambda r, k: O.loglik_css(r, S.p, S.d, S.q, 1, k), s, c))


def fam_css_gradient(e, N):
    s, c = _data(N)
    y = np.ascontiguousarray(np.diff(s, axis=1))
    assert _same(e.css_gradient(y, S.p, S.q, True, c), np.stack(_each(lambda r, k: O.gradient_css_arma(r, S.p, S.q, 1, k), y, c)))


def fam_hannan_rissanen(e, N):
    s, _ = _data(N)
    y = np.ascontiguousarray(np.diff(s, axis=1))
    init, st = e.hannan_rissanen(y, S.p, S.q, True)
    for i in range(N):
        est, eini = O.hannan_rissanen(y[i], S.p, S.q, 1)
        assert st[i] == est and (est != 0 or _same(init[i], eini)), i


def fam_model_flags(e, N):
    _, c = _data(N)
    assert np.array_equal(e.model_flags(c * 3.0, S.p, S.q, True), [O.model_flags(k, S.p, S.q, 1) for k in c * 3.0])


def fam_forecast(e, N):
    s, c = _data(N)
    assert _same(e.forecast(s, S.p, S.d, S.q, True, c, S.nf),
                 np.stack(_each(lambda r, k: O.forecast(r, S.p, S.d, S.q, 1, k, S.nf), s, c)))


def fam_effects(e, N):
    s, c = _data(N)
    for host, ref in ((e.remove_effects, O.remove_time_dependent_effects), (e.add_effects, O.add_time_dependent_effects)):
        exp = np.stack(_each(lambda r, k: ref(r, S.p, S.d, S.q, 1, k), s, c))
        assert _same(host(s, S.p, S.d, S.q, True, c), exp)
        rows = s.copy()
        assert host(rows, S.p, S.d, S.q, True, c, out=rows) is rows and _same(rows, exp), "in place"


def fam_diagnostics(e, N):
    s, _ = _data(N)
    diag_check(e.diagnostics(s, S.lag), diag_ref(s, S.lag), f"N {N}")


def _resid(s, c):
    return np.stack(_each(lambda r, k: O.remove_time_dependent_effects(r, S.p, S.d, S.q, 1, k), s, c))


def fam_residual_diagnostics(e, N):
    s, c = _data(N)
    diag_check(e.residual_diagnostics(s, S.p, S.d, S.q, True, c, S.lag), diag_ref(_resid(s, c), S.lag), f"N {N}")


def fam_order_search(e, N):
    s, _ = _data(N)
    order, coef, aic = e.order_search(s, 2, 1, 2, 2)
    eo, ec, ea = O.order_search(s, 2, 1, 2, 2)
    assert np.array_equal(order, eo) and _same(aic, ea) and _same(coef, ec), (order, eo)


def fam_autofit(e, N):
    s, _ = _data(N)
    exp = [O.autofit(r, 2, 1, 2) for r in s]
    check_autofit(e.autofit(s, 2, 1, 2), {k: np.array([x[k] for x in exp]) for k in ("status", "order", "n_fits", "coef", "aic")},
                  f"N {N}")


def fam_kpss(e, N):
    s, _ = _data(N)
    stat, st = e.kpss(s)
    exp = [O.kpss(r, "c") for r in s]
    assert np.array_equal(st, [x[0] for x in exp]) and _same(stat, np.array([x[1] for x in exp]))


def _ewma_exp(s):
    return R.fit_batch(s.tolist(), "ewma")


def _check_ewma(r, exp):
    assert _same(r["smoothing"], exp["coef"][:, 0]) and _same(r["sse"], exp["obj"])
    assert all(_same(r[k], exp[k]) for k in ("status", "n_eval", "n_grad"))


def fam_model_fit(e, N):
    s, _ = _data(N)
    _check_ewma(e.ewma_fit_batch(s), _ewma_exp(s))
    g = np.diff(s, axis=1, prepend=0.0) * 0.3
    r, exp = e.garch_fit_batch(g), R.fit_batch(g.tolist(), "garch")
    assert _same(r["coef"], exp["coef"]) and _same(r["ll"], exp["obj"])
    assert all(_same(r[k], exp[k]) for k in ("status", "n_eval", "n_grad"))


SM = np.array([0.3, 0.94, 1.2, 0.5, 0.05])
GC = np.array([[.2, .3, .4], [.1, .2, .3], [.3, .1, .5], [.25, .35, .3], [.05, .4, .4]])


def fam_model_eval(e, N):
    s, _ = _data(N)
    rows, sm, g = s.tolist(), SM[:N].tolist(), GC[:N].tolist()
    assert _same(e.ewma_sse(s, SM[:N]), _each(R.ewma_sse, rows, sm))
    assert _same(e.ewma_gradient(s, SM[:N]), _each(R.ewma_gradient, rows, sm))
    assert _same(e.garch_loglik(s, GC[:N]), [R.garch_loglik(r, *c) for r, c in zip(rows, g)])
    assert _same(e.garch_gradient(s, GC[:N]), np.array([R.garch_gradient(r, *c) for r, c in zip(rows, g)]))


def fam_model_effects(e, N):
    s, _ = _data(N)
    rows, sm, g = s.tolist(), SM[:N].tolist(), GC[:N].tolist()
    assert _same(e.ewma_remove_effects(s, SM[:N]), np.array(_each(R.ewma_remove, rows, sm)))
    assert _same(e.ewma_add_effects(s, SM[:N]), np.array(_each(R.ewma_add, rows, sm)))
    assert _same(e.garch_remove_effects(s, GC[:N]), np.array([R.garch_remove(r, *c) for r, c in zip(rows, g)]))
    assert _same(e.garch_add_effects(s, GC[:N]), np.array([R.garch_add(r, *c) for r, c in zip(rows, g)]))


def fam_regress(e, N):
    s, _ = _data(N)
    x = np.random.default_rng(20261021).standard_normal((5, S.T, RG.k))[:N]
    fits = [RR.arx_fit(s[i], x[i].T, RG.yl, RG.xl, True, False) for i in range(N)]
    coef = np.array([[c] + list(cf) for _, c, cf in fits])
    got = e.arx_fit(s, x, RG.yl, RG.xl, True, False)
    assert np.all(got["status"] == RR.ST_OK) and np.array_equal(got["status"], [f[0] for f in fits])
    assert coef.shape == (N, 1 + RG.K) and _same(got["coef"], coef)
    pred = np.array([RR.arx_predict(s[i], x[i].T, coef[i, 0], coef[i, 1:], RG.yl, RG.xl, True) for i in range(N)])
    assert pred.shape == (N, RG.R) and _same(e.arx_predict(s, x, RG.yl, RG.xl, True, coef), pred)
    for got, ref in ((e.bgtest(s, x, S.lag), [RR.bgtest(s[i], x[i].T, S.lag) for i in range(N)]),
                     (e.bptest(s, x), [RR.bptest(s[i], x[i].T) for i in range(N)])):
        assert np.all(got["status"] == RR.ST_OK) and np.array_equal(got["status"], [r[0] for r in ref])
        assert _same(got["stat"], np.array([r[1] for r in ref])) and _p_close(got["pvalue"], [r[2] for r in ref])


def _xreg(N, rows):
    return np.random.default_rng(20261021).standard_normal((5, rows, RG.k))[:N]


def fam_regarima(e, N):
    s, _ = _data(N)
    x = _xreg(N, S.T)
    coef, rho, n_iter, status = CO.fit_batch(s, x, 5)[:4]
    got = e.regarima_co_fit(s, x, 5)
    assert np.all(got["status"] == RR.ST_OK) and np.array_equal(got["status"], status)
    assert np.array_equal(got["n_iter"], n_iter) and _same(got["rho"], rho) and _same(got["coef"], np.array(coef))


def fam_arimax(e, N):
    s, _ = _data(N)
    x, xf = _xreg(N, S.T), _xreg(N, S.nf)

    def cols(m):
        return m.transpose(0, 2, 1).tolist()

    for d in (0, 1):
        ref = AXR.arimax_fit_batch(s, cols(x), AX.p, d, AX.q, AX.L, True, True, smear=e.get_option("smear"))
        got = e.arimax_fit(s, x, AX.p, d, AX.q, AX.L, True, True)
        assert ref["coef"].shape == (N, AX.Kp) and _same(got["coef"], ref["coef"]) and _same(got["ll"], ref["ll"])
        assert all(np.array_equal(got[k], ref[k]) for k in ("status", "n_eval", "n_grad"))
        coef = np.where(np.isnan(ref["coef"]), 0.1, ref["coef"])
        assert _same(e.arimax_forecast(s, xf, AX.p, d, AX.q, AX.L, True, True, coef),
                     AXR.arimax_forecast_batch(s, cols(xf), AX.p, d, AX.q, AX.L, True, True, coef))


FAMILIES = [fam_difference, fam_css_loglik, fam_css_gradient, fam_hannan_rissanen, fam_model_flags, fam_forecast,
            fam_effects, fam_diagnostics, fam_residual_diagnostics, fam_order_search, fam_autofit, fam_kpss,
            fam_model_fit, fam_model_eval, fam_model_effects, fam_regress, fam_regarima, fam_arimax]


@pytest.fixture
def fresh(engine):
    """A handle that has staged nothing yet."""
    e = L.Engine(engine.device)
    yield e
    assert e.L.arima_destroy(e.h) == OK


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__[4:])
def test_valid_calls_three_then_five_series(fresh, family):
    family(fresh, 3)
    family(fresh, 5)


def test_different_staging_tables_back_to_back(fresh):
    s, c = _data(5)
    exp_diag, exp_ewma = diag_ref(_resid(s, c), S.lag), _ewma_exp(s)
    exp_fc = np.stack(_each(lambda r, k: O.forecast(r, S.p, S.d, S.q, 1, k, S.nf), s, c))
    x = _xreg(5, S.T)
    exp_co = CO.fit_batch(s, x, 5)
    exp_ax = AXR.arimax_fit_batch(s, x.transpose(0, 2, 1).tolist(), AX.p, AX.d, AX.q, AX.L, True, True,
                                  smear=fresh.get_option("smear"))
    for _ in range(2):
        diag_check(fresh.residual_diagnostics(s, S.p, S.d, S.q, True, c, S.lag), exp_diag, "sequence")
        ax = fresh.arimax_fit(s, x, AX.p, AX.d, AX.q, AX.L, True, True)                     # 8 staged arrays
        assert _same(ax["coef"], exp_ax["coef"]) and np.array_equal(ax["n_eval"], exp_ax["n_eval"])
        _check_ewma(fresh.ewma_fit_batch(s), exp_ewma)
        co = fresh.regarima_co_fit(s, x, 5)                                                 # 6
        assert _same(co["coef"], np.array(exp_co[0])) and np.array_equal(co["n_iter"], exp_co[2])
        assert _same(fresh.forecast(s, S.p, S.d, S.q, True, c, S.nf), exp_fc)


def test_device_effects_in_place_equals_out_of_place(engine):
    import torch
    s, c = _data(S.N)
    dev = f"cuda:{engine.device}"
    cd = torch.from_numpy(c).to(dev)
    for which in ("remove", "add"):
        rows = torch.full((S.N, S.ld), -7.0, dtype=torch.float64, device=dev)
        rows[:, :S.T] = torch.from_numpy(s).to(dev)
        out = torch.full((S.N, S.ldo), -7.0, dtype=torch.float64, device=dev)
        run = getattr(engine, f"{which}_effects_device")
        run(rows.data_ptr(), S.N, S.T, S.ld, S.p, S.d, S.q, S.I, cd.data_ptr(), out.data_ptr(), S.ldo)
        run(rows.data_ptr(), S.N, S.T, S.ld, S.p, S.d, S.q, S.I, cd.data_ptr(), rows.data_ptr(), S.ld)
        assert torch.equal(rows[:, :S.T], out[:, :S.T])
        assert bool((rows[:, S.T:] == -7.0).all()) and bool((out[:, S.T:] == -7.0).all())
