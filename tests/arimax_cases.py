"""Inputs shared by the ARIMAX tests (TEST INFRASTRUCTURE): the reference suite's data (tests/golden/arimax) and the
synthetic batches of the device tests, with their restated fits computed once per process."""
import functools
import json
import os

import numpy as np

import arimax_ref as AX

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arimax")


def _load(name):
    with open(os.path.join(_GOLDEN, name)) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def suite_data():
    """ARIMAXSuite's two data sets: {1, 2} -> (tsTrain, xregTrain columns, tsTest, xregTest columns)."""
    tr, te, inl = _load("data_train.json"), _load("data_test.json"), _load("inline.json")

    def cols(flat, rows, ncols):
        return [flat[c * rows:(c + 1) * rows] for c in range(ncols)]

    return {1: (tr["gdp"], [tr["sales"], tr["ad_budget"]], te["gdp"], [te["sales"], te["ad_budget"]]),
            2: (inl["ts_train_2"], cols(inl["xreg_train_2"], inl["xreg_train_2_rows"], inl["xreg_train_2_cols"]),
                inl["ts_test_2"], cols(inl["xreg_test_2"], inl["xreg_test_2_rows"], inl["xreg_test_2_cols"]))}


def suite_cases():
    return _load("cases.json")


@functools.lru_cache(maxsize=None)
def suite_fit(idx, smear):
    c = suite_cases()[idx]
    ts, x, _, _ = suite_data()[c["data"]]
    return AX.arimax_fit(ts, x, c["p"], c["d"], c["q"], c["xreg_max_lag"], c["include_original_xreg"],
                         c["include_intercept"], smear=smear)


# ---- the device tests' batches ------------------------------------------------------------------------------------
# (p, d, q, L, includeOriginal, intercept, T, k)
CONFIGS = {"a": (1, 0, 1, 1, True, True, 40, 2), "b": (2, 1, 1, 1, True, False, 48, 2),
           "c": (0, 0, 2, 2, False, True, 40, 1), "d": (1, 1, 2, 0, True, True, 64, 3)}
N_MAX = 130
PHIS = (0.0, 0.4, 0.8, -0.6)
THETAS = (0.0, 0.5, -0.4)


@functools.lru_cache(maxsize=None)
def batch(cfg, shared_x=False):
    """(series N_MAX x T, x N_MAX x T x k or T x k): y = 5 + 1.5 x0 - 0.7 x1 + ARMA(1, 1) errors with phi and theta
    drawn per series; x = 0.3 random walk + noise (columns past the second carry no weight)."""
    p, d, q, L, orig, icpt, T, k = CONFIGS[cfg]
    rng = np.random.default_rng(20 + ord(cfg))
    nx = 1 if shared_x else N_MAX
    x = 0.3 * np.cumsum(rng.standard_normal((nx, T, k)), axis=1) + rng.standard_normal((nx, T, k))
    y = np.empty((N_MAX, T))
    for i in range(N_MAX):
        phi, theta = PHIS[rng.integers(len(PHIS))], THETAS[rng.integers(len(THETAS))]
        e = rng.standard_normal(T + 1)
        u = np.empty(T)
        prev = 0.0
        for t in range(T):
            prev = phi * prev + e[t + 1] + theta * e[t]
            u[t] = prev
        xi = x[0 if shared_x else i]
        y[i] = 5.0 + 1.5 * xi[:, 0] - (0.7 * xi[:, 1] if k > 1 else 0.0) + u
    return y, (x[0] if shared_x else x)


def x_columns(x):
    """(T, k) or (N, T, k) -> the restatement's lists of columns."""
    x = np.asarray(x)
    return x.T.tolist() if x.ndim == 2 else x.transpose(0, 2, 1).tolist()


@functools.lru_cache(maxsize=None)
def batch_ref(cfg, smear, shared_x=False):
    """arimax_ref's fits of batch(cfg) under `smear`."""
    p, d, q, L, orig, icpt, T, k = CONFIGS[cfg]
    y, x = batch(cfg, shared_x)
    return AX.arimax_fit_batch(y, x_columns(x), p, d, q, L, orig, icpt, smear=smear)


@functools.lru_cache(maxsize=None)
def user_init_case():
    """Config "a", 65 series, from a start that is not the one fitModel would build."""
    p, d, q, L, orig, icpt, T, k = CONFIGS["a"]
    y, x = (v[:65] for v in batch("a"))
    init = np.random.default_rng(3).uniform(-0.3, 0.3, (65, AX.num_coef(k, p, q, L, orig)))
    init[:, 0] = 5.0
    return y, x, init, AX.arimax_fit_batch(y, x_columns(x), p, d, q, L, orig, icpt, user_init=init)


# ---- failing lanes next to healthy ones: lanes 0 and 63 of the first wave, lane 0 of the second ----------------------
EDGE_LANES = {"ones-column": 0, "nan-series": 63, "ones-column-2": 64}


@functools.lru_cache(maxsize=None)
def edge_batch():
    """Config "a", 70 series: a ones column in x (collinear with the ARX intercept: SINGULAR) and a series of NaN."""
    p, d, q, L, orig, icpt, T, k = CONFIGS["a"]
    y, x = (v[:70].copy() for v in batch("a"))
    x[EDGE_LANES["ones-column"], :, 1] = 1.0
    x[EDGE_LANES["ones-column-2"], :, 0] = 1.0
    y[EDGE_LANES["nan-series"]] = np.nan
    return y, x, AX.arimax_fit_batch(y, x_columns(x), p, d, q, L, orig, icpt)


# series too short, the same for every series of a call: (p, d, q, L, includeOriginal, intercept, T, k) -> the status
# of the ARX regression alone and of Hannan-Rissanen alone (0 = fine); the fit reports the first that is not 0
SHORT_CASES = {
    "arx-too-short": ((1, 0, 1, 8, True, True, 7, 2), 10, 0),       # T - max(p, L) < 0; Hannan-Rissanen is fine
    "arx-not-enough": ((1, 0, 1, 1, True, True, 6, 2), 5, 0),       # 6 predictors + 1 > 5 rows
    "hr-not-enough": ((0, 0, 3, 0, True, True, 8, 1), 0, 5),        # the AR(4) stage: 4 + 1 > 4 rows; the ARX is fine
    "both-arx-wins": ((1, 5, 1, 1, True, True, 6, 2), 5, 10),       # ARX on the 6 raw values, Hannan-Rissanen on 1
}


@functools.lru_cache(maxsize=None)
def short_case(name):
    (p, d, q, L, orig, icpt, T, k), _, _ = SHORT_CASES[name]
    rng = np.random.default_rng(len(name))
    y, x = rng.standard_normal((66, T)), rng.standard_normal((66, T, k))
    return y, x, AX.arimax_fit_batch(y, x_columns(x), p, d, q, L, orig, icpt)


# K' at the library's limit (kGenMaxK = 41): 1 + 2 + 2 + 6 * 5 + 6
WIDE = (2, 0, 2, 5, True, True, 60, 6)


@functools.lru_cache(maxsize=None)
def wide_case():
    p, d, q, L, orig, icpt, T, k = WIDE
    rng = np.random.default_rng(41)
    x = rng.standard_normal((3, T, k))
    y = 2.0 + x[:, :, 0] + 0.5 * rng.standard_normal((3, T))
    return y, x, AX.arimax_fit_batch(y, x_columns(x), p, d, q, L, orig, icpt)


# ---- forecasts -----------------------------------------------------------------------------------------------------
FC_N = 65
FC_T = (31, 32, 33, 65)
FC_NF = ("1", "16", "T", "T+L")
FC_D = (0, 1, 2)
FC_ORDERS = ((1, 1), (2, 1), (0, 2), (2, 0), (1, 2))
# (includeOriginal, L, intercept): every combination with at least one predictor, and the one without any
FC_FLAGS = tuple((o, L, i) for o in (True, False) for L in (0, 1, 2) for i in (True, False))


def n_future_of(rule, T, L):
    return {"1": 1, "16": 16, "T": T, "T+L": T + L}[rule]


def forecast_shapes():
    """Every (T, nFuture rule, d) with two of the twelve flag combinations, rotating through them, the orders and
    k in {2, 3, 1}; a shape the reference throws for (nFuture = 1 under d = 2 leaves max(p, q) rows, fewer than L = 2
    at order (1, 1)) is left to the invalid-shape tests."""
    out = []
    i = 0
    for T in FC_T:
        for rule in FC_NF:
            for d in FC_D:
                for j in (0, 1):
                    flags, (p, q), k = FC_FLAGS[(5 * i + 7 * j) % 12], FC_ORDERS[(i + j) % 5], (2, 3, 1)[(i + j) % 3]
                    try:
                        AX.forecast_check(T, k, n_future_of(rule, T, flags[1]), p, d, q, flags[1])
                    except ValueError:
                        continue
                    out.append((T, rule, d, flags, (p, q), k))
                i += 1
    return out


# orders above the compiled forecast's (p or q > 5, d > 8): the workspace kernel; same tuples as forecast_shapes()
FC_WORKSPACE_SHAPES = [(33, "16", 1, (True, 1, True), (6, 1), 2), (32, "T", 0, (False, 2, False), (0, 7), 3),
                       (31, "1", 2, (True, 0, True), (7, 6), 1), (40, "16", 9, (True, 1, True), (1, 1), 2),
                       (65, "T+L", 1, (False, 1, True), (2, 6), 2)]


@functools.lru_cache(maxsize=None)
def forecast_case(shape):
    """(series, x (N, nFuture, k), coef (N, K'), restated forecasts). Every fifth series has NaN and +-Inf in the
    columns 0 .. k-2, which the reference multiplies and drops; series 7 and 8 carry a NaN and an Inf in xreg
    coefficients the forecast never reads (every one but coefficient p + q + k), series 9 and 10 in ones it reads."""
    T, rule, d, (orig, L, icpt), (p, q), k = shape
    nF = n_future_of(rule, T, L)
    rng = np.random.default_rng([T, nF, d, int(orig), L, int(icpt), p, q, k])
    Kp = AX.num_coef(k, p, q, L, orig)
    y = np.cumsum(rng.standard_normal((FC_N, T)), axis=1) + 10.0
    x = rng.standard_normal((FC_N, nF, k)) + 3.0
    coef = rng.uniform(-0.5, 0.5, (FC_N, Kp))
    if k > 1:
        x[::5, nF // 2, 0] = np.nan
        x[5::10, 0, k - 2] = np.inf
        x[::10, nF - 1, k - 2] = -np.inf
    if Kp > 1 + p + q + k:                           # more than k xreg coefficients: some are never read
        coef[7, 1 + p + q + (0 if k > 1 else 1)] = np.nan
        coef[8, Kp - 1] = np.inf
    coef[9, 1] = np.nan
    coef[10, 0] = -np.inf
    ref = AX.arimax_forecast_batch(y, x_columns(x), p, d, q, L, orig, icpt, coef)
    return y, x, coef, ref


# ---- a forecast batch larger than one workspace slice ---------------------------------------------------------------
def forecast_ws(T, d, M, n_future):
    """Doubles of workspace per series of the runtime-order ARIMAX forecast (csrc: arimax_forecast_ws_doubles)."""
    n = T - d
    hist_len, fl, tn = M + n, n_future + M, max(T, n_future)
    return (2 * (tn + 1) + 2 * (hist_len + 1) + (fl + 1) + (d + 1) * T + 2 * (d + n_future + 1)
            + (T + n_future + 1) + (n_future + 1) + (fl + 1))


def forecast_slice(N, T, p, d, q, n_future):
    """Series per launch of the workspace kernel (arima_runtime.cpp): max(1, min(N, 2^27 / w))."""
    return max(1, min(N, (1 << 27) // max(forecast_ws(T, d, max(p, q), n_future), 1)))


# d = 9 takes the workspace kernel at any p, q; nFuture above d, or no predictor row exists and x is never read
SLICE_SHAPE = (512, 13, 9, (True, 1, True), (1, 1), 2)         # T, nFuture, d, (includeOriginal, L, intercept), (p, q), k
SLICE_N = (1 << 27) // forecast_ws(512, 9, 1, 13) + 65
SLICE_WINDOW = 64                                                # rows on each side of the boundary forecast alone
SLICE_REF = 4                                                    # rows on each side held to the restatement


@functools.lru_cache(maxsize=None)
def slice_case():
    """(series N x T, x N x nFuture x k, coef N x K', sl, restated forecasts of rows [sl - 4, sl + 4)): one matrix and
    one model per series, every row drawn on its own, so rows a slice apart differ in all three."""
    T, nF, d, (orig, L, icpt), (p, q), k = SLICE_SHAPE
    rng = np.random.default_rng(271828)
    y = np.cumsum(rng.standard_normal((SLICE_N, T)), axis=1) + 10.0
    x = rng.standard_normal((SLICE_N, nF, k)) + 3.0
    coef = rng.uniform(-0.5, 0.5, (SLICE_N, AX.num_coef(k, p, q, L, orig)))
    sl = forecast_slice(SLICE_N, T, p, d, q, nF)
    r = slice(sl - SLICE_REF, sl + SLICE_REF)
    ref = AX.arimax_forecast_batch(y[r], x_columns(x[r]), p, d, q, L, orig, icpt, coef[r])
    for a in (y, x, coef, ref):
        a.setflags(write=False)
    return y, x, coef, sl, ref
