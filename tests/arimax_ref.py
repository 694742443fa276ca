"""CPU restatement of ARIMAX.fitModel and ARIMAXModel.forecast (models/ARIMAX.scala) -- TEST INFRASTRUCTURE.

Composed from the restatements that already exist: oracle (differencing, hannan_rissanen, the CSS log-likelihood and
its gradient with the `smear` reading of DESIGN.md 5.1), regress_ref.arx_fit (AutoregressionX.fitModel) and
smallfit_ref.cg_optimize (commons' NonLinearConjugateGradientOptimizer), plus the two pieces only ARIMAX has: the
inert gradient columns and the forecast's xreg term. Python floats are IEEE doubles and never fuse a * b + c. The
device code (csrc/arima_arimax.hip) is held to this file bit for bit.

A regressor matrix is a list of k columns (the column-major DenseMatrix(rows, k)), as in regress_ref.

The coefficient vector has K' = 1 + p + q + nX entries: slot 0 exists even without an intercept (it then starts at
0.0). The objective and the gradient read only the first ka = I + p + q of them, in ARIMA's layout
`coefficients(intercept + j)` (ARIMAX.scala:266-370); the forecast reads `coefficients(1 + j)` whatever the
intercept flag says (:479-541). Both are kept.
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(os.path.dirname(_HERE), "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import oracle as O  # noqa: E402
import regress_ref as R  # noqa: E402
import smallfit_ref as S  # noqa: E402

NAN = float("nan")
ST_OK = 0


def num_xcoef(k, xreg_max_lag, include_original_xreg):
    return k * xreg_max_lag + (k if include_original_xreg else 0)


def num_coef(k, p, q, xreg_max_lag, include_original_xreg=True):
    """K' = coefficients.length of a fitted model (the suite asserts 6, 11, 10, 8, 11, 12)."""
    return 1 + p + q + num_xcoef(k, xreg_max_lag, include_original_xreg)


def _cols(x):
    return [[float(v) for v in col] for col in x]


def difference_xreg_flat(x, d):
    """estimateARXCoefficients (:98-102): the whole column-major matrix differenced as ONE vector of k * T values and
    cut back into columns: the first d values stay, column c >= 1 starts with a difference against column c - 1."""
    x = _cols(x)
    k = len(x)
    T = len(x[0]) if k else 0
    flat = [v for col in x for v in col]
    if not flat:
        return x
    diffed = O.differences_of_order_d(np.asarray(flat), d).tolist()
    return [diffed[c * T:(c + 1) * T] for c in range(k)]


def arimax_init(ts, x, p, d, q, xreg_max_lag, include_original_xreg=True, include_intercept=True):
    """fitModel's start point (:72-80): (status, init of K' values). The ARX regression runs first, on the
    UNDIFFERENCED series and the flat-differenced matrix, always with an intercept; then Hannan-Rissanen on the
    differenced series, whose last q values are the MA part (it runs, and can throw, with q = 0 too)."""
    ts = [float(v) for v in ts]
    Kp = num_coef(len(x), p, q, xreg_max_lag, include_original_xreg)
    st, c, coefs = R.arx_fit(ts, difference_xreg_flat(x, d), p, xreg_max_lag, include_original_xreg, False)
    if st != ST_OK:
        return st, [NAN] * Kp
    arx = [c if include_intercept else 0.0] + list(coefs)
    diffed = O.differences_of_order_d(np.asarray(ts), d)[d:]
    st, hr = O.hannan_rissanen(diffed, p, q, include_intercept)
    if st != ST_OK:
        return st, [NAN] * Kp
    ma = [float(v) for v in hr[len(hr) - q:]] if q > 0 else []
    return ST_OK, arx[:p + 1] + ma + arx[p + 1:]


def inert_gradient(diffed, p, q, I, c, smear=O.DEFAULT_SMEAR):
    """One column j >= ka of gradientlogLikelihoodCSSARMA (:301-370), operation by operation. Such a column of dEdTheta
    only ever receives `dEdTheta(0, j) -= coefficients(intercept + p + k) * dEdTheta(k + 1, j)`, the gradient
    `+= dEdTheta(0, j) * error`, the lag rows the overlapping copy of :362 (`smear`) and the division by -sigma2. Every
    inert column sees the same operands in the same order, so one is computed for all of them."""
    y = [float(v) for v in diffed]
    n = len(y)
    M = max(p, q)
    dE0 = 0.0
    lag = [0.0] * q                                   # dEdTheta(1 .. q, j)
    ma = [0.0] * q
    g = 0.0
    sigma2 = 0.0
    for i in range(M, n):
        for k in range(q):
            dE0 = dE0 - c[I + p + k] * lag[k]
        yhat = 0.0 + float(I) * c[0]
        for j in range(p):
            yhat = yhat + y[i - j - 1] * c[I + j]
        for j in range(q):
            yhat = yhat + ma[j] * c[I + p + j]
        e = y[i] - yhat
        sigma2 = sigma2 + S.jdiv(e * e, float(n))
        for j in range(q - 1):                        # updateMAErrors: the ascending copy
            ma[j + 1] = ma[j]
        if q > 0:
            ma[0] = e
        g = g + dE0 * e
        if smear:
            for r in range(q):
                lag[r] = dE0 if r == 0 else lag[r - 1]
        else:
            for r in range(q - 1, 0, -1):
                lag[r] = lag[r - 1]
            if q > 0:
                lag[0] = dE0
        dE0 = 0.0
    return S.jdiv(g, -sigma2)


def gradient_literal(diffed, p, q, I, c, smear=O.DEFAULT_SMEAR):
    """gradientlogLikelihoodCSSARMA (:301-370) over all coefficients.length columns, written down as it stands (slow:
    the fit uses gradient(); tests hold the two to each other)."""
    y = [float(v) for v in diffed]
    n, K = len(y), len(c)
    M = max(p, q)
    dE = [[0.0] * K for _ in range(q + 1)]
    g = [0.0] * K
    ma = [0.0] * q
    sigma2 = 0.0
    for i in range(M, n):
        for j in range(K):
            for k in range(q):
                dE[0][j] = dE[0][j] - c[I + p + k] * dE[k + 1][j]
        yhat = 0.0 + float(I) * c[0]
        dE[0][0] = dE[0][0] - float(I)
        for j in range(p):
            yhat = yhat + y[i - j - 1] * c[I + j]
            dE[0][I + j] = dE[0][I + j] - y[i - j - 1]
        for j in range(q):
            yhat = yhat + ma[j] * c[I + p + j]
            dE[0][I + p + j] = dE[0][I + p + j] - ma[j]
        e = y[i] - yhat
        sigma2 = sigma2 + S.jdiv(e * e, float(n))
        for j in range(q - 1):
            ma[j + 1] = ma[j]
        if q > 0:
            ma[0] = e
        for j in range(K):
            g[j] = g[j] + dE[0][j] * e
        if smear:
            for r in range(1, q + 1):
                dE[r] = list(dE[r - 1])
        else:
            for r in range(q, 0, -1):
                dE[r] = list(dE[r - 1])
        dE[0] = [0.0] * K
    return [S.jdiv(v, -sigma2) for v in g]


def gradient(diffed, p, q, I, c, smear=O.DEFAULT_SMEAR):
    """The K' gradient: the ka active columns are ARIMA's (oracle.gradient_css_arma on the coefficient prefix), the
    others inert_gradient."""
    ka = I + p + q
    active = O.gradient_css_arma(diffed, p, q, I, c[:ka], smear).tolist() if ka else []
    if len(c) == ka:
        return active
    return active + [inert_gradient(diffed, p, q, I, c, smear)] * (len(c) - ka)


def loglik(diffed, p, q, I, c):
    """logLikelihoodCSSARMA (:266-281): ARIMA's, over the first ka coefficients."""
    return O.loglik_css_arma(diffed, p, q, I, c[:max(I + p + q, 1)])


def arimax_fit(ts, x, p, d, q, xreg_max_lag, include_original_xreg=True, include_intercept=True, user_init=None,
               smear=O.DEFAULT_SMEAR):
    """ARIMAX.fitModel (:59-87): dict(status, coef K', ll, n_eval, n_grad, n_iter, init). The optimizer runs over all
    K' coordinates (its restart period `iter % n` is K'); a failed fit has NaN coefficients and ll."""
    I = 1 if include_intercept else 0
    ts = np.ascontiguousarray(ts, dtype=np.float64)
    diffed = O.differences_of_order_d(ts, d)[d:]
    if user_init is None:
        st, init = arimax_init(ts, x, p, d, q, xreg_max_lag, include_original_xreg, include_intercept)
        if st != ST_OK:
            return dict(status=st, coef=[NAN] * len(init), ll=NAN, n_eval=0, n_grad=0, n_iter=0, init=init)
    else:
        init = [float(v) for v in user_init]
    r = S.cg_optimize(lambda c: loglik(diffed, p, q, I, c), lambda c: gradient(diffed, p, q, I, c, smear), init, 1e-7,
                      False)
    return dict(status=r["status"], coef=r["x"], ll=r["obj"], n_eval=r["n_eval"], n_grad=r["n_grad"],
                n_iter=r["n_iter"], init=init)


def _x_of(x, i):
    """Series i's matrix: x is one matrix (a list of columns) or a list of N of them."""
    return x[i] if np.ndim(x) == 3 else x


def arimax_fit_batch(series, x, p, d, q, xreg_max_lag, include_original_xreg=True, include_intercept=True,
                     user_init=None, smear=O.DEFAULT_SMEAR):
    """Fits of every row; x shared (k columns) or per series (N x k columns). dict(coef N x K', ll, status, n_eval,
    n_grad, n_iter, init N x K')."""
    series = np.ascontiguousarray(series, dtype=np.float64)
    N = series.shape[0]
    Kp = num_coef(len(_x_of(x, 0)), p, q, xreg_max_lag, include_original_xreg)
    out = dict(coef=np.empty((N, Kp)), init=np.empty((N, Kp)), ll=np.empty(N), status=np.empty(N, np.int32),
               n_eval=np.empty(N, np.int32), n_grad=np.empty(N, np.int32), n_iter=np.empty(N, np.int32))
    for i in range(N):
        r = arimax_fit(series[i], _x_of(x, i), p, d, q, xreg_max_lag, include_original_xreg, include_intercept,
                       None if user_init is None else np.asarray(user_init, dtype=np.float64).reshape(-1, Kp)[
                           i if np.ndim(user_init) > 1 else 0], smear)
        out["coef"][i], out["init"][i], out["ll"][i] = r["coef"], r["init"], r["ll"]
        out["status"][i], out["n_eval"][i], out["n_grad"][i], out["n_iter"][i] = (r["status"], r["n_eval"],
                                                                                  r["n_grad"], r["n_iter"])
    return out


# ---- ARIMAXModel.forecast (:201-256) ----------------------------------------------------------------------------
def difference_xreg(x, d, M):
    """differenceXreg (:552-561): every column on its own, d values dropped, M zeros in front."""
    return [[0.0] * M + O.differences_of_order_d(np.asarray(col, dtype=np.float64), d)[d:].tolist() for col in x]


def forecast_check(T, k, n_future, p, d, q, xreg_max_lag):
    """The shapes for which the reference throws for every series (ValueError here, ARIMA_E_INVALID_ARG in the C ABI):
      M = 0                xregPredictors(maxPQ - 1) is xregPredictors(-1) (:515)
      k = 0                `exogenousVar.flatten.length / exogenousVar.size` divides by zero (:495)
      T < d                the slices of steps [5] and [7], as in ARIMAModel.forecast
      R - L < 0            Lag.lagMatTrimBoth sizes a matrix of R - L rows; R = M + max(nFuture - d, 0) is the length
                           of a differenced, zero-prefixed column (nFuture >= d: M + nFuture - d)
      R - L > M + T - d    assemblePredictors' transpose sizes its rows by the first array (the tsSize = M + T - d empty
                           AR rows) and overruns on the R - L predictor rows (nFuture >= d: nFuture - L > T)
    """
    M = max(p, q)
    R_ = M + max(n_future - d, 0)
    if min(T, k, n_future, p, d, q, xreg_max_lag) < 0:
        raise ValueError("negative shape")
    if M == 0:
        raise ValueError("max(p, q) = 0: xregPredictors(-1)")
    if k == 0:
        raise ValueError("no xreg columns: division by zero")
    if T < d:
        raise ValueError("series shorter than d")
    if R_ - xreg_max_lag < 0:
        raise ValueError("fewer differenced xreg rows than xregMaxLag")
    if R_ - xreg_max_lag > M + T - d:
        raise ValueError("more predictor rows than history: transpose overruns")
    return M, R_


def arimax_forecast(ts, x, p, d, q, xreg_max_lag, include_original_xreg, include_intercept, coef):
    """ARIMAXModel.forecast(ts, xreg): the LAST T of the T + nFuture values (`results.drop(nFuture)`, :254); x: k
    columns of nFuture values. The xreg term of a step is an assignment inside the loop over the predictor row (:522):
    only the row's last predictor survives, times coefficients(p + q + k); the rest of the row is multiplied and
    dropped, so columns 0 .. k-2 never reach the output."""
    ts = [float(v) for v in ts]
    c = [float(v) for v in coef]
    x = _cols(x)
    T, k = len(ts), len(x)
    nF = len(x[0]) if k else 0
    L = xreg_max_lag
    M, R_ = forecast_check(T, k, nF, p, d, q, L)
    I = 1 if include_intercept else 0
    xd = difference_xreg(x, d, M)
    last = xd[k - 1]
    w = c[p + q + k] if (L > 0 or include_original_xreg) else 0.0

    def impact(i):
        """xregImpact of loop index i (`maxPQ`): predictor row i - 1, empty from row R - L on."""
        r = i - 1
        if r >= R_ - L or not (L > 0 or include_original_xreg):
            return 0.0
        # the other predictors of the row: multiplied, then overwritten (a NaN there never shows)
        return (last[r + L] if include_original_xreg else last[r]) * w

    def iterate(tsv, hist, ma):
        for i in range(M, len(tsv)):
            hist[i] = hist[i] + float(I) * c[0]
            for j in range(p):
                if i - j - 1 >= 0:
                    hist[i] = hist[i] + tsv[i - j - 1] * c[1 + j]
            hist[i] = hist[i] + impact(i)
            for j in range(q):
                hist[i] = hist[i] + ma[j] * c[1 + p + j]
            e = tsv[i] - hist[i]
            for j in range(len(ma) - 1):                    # updateMAErrors
                ma[j + 1] = ma[j]
            if ma:
                ma[0] = e

    intercept = c[0] if I else 0.0
    dts = O.differences_of_order_d(np.asarray(ts), d)[d:].tolist()
    ext = [intercept] * M + dts                                                   # [1]
    hl = len(ext)
    hist = [0.0] * hl                                                             # [2]
    iterate(ext, hist, [0.0] * q)
    ma_terms = [ext[i] - hist[i] for i in range(hl - M, hl)]                      # [3]
    fwd = [0.0] * (nF + M)                                                        # [4]
    fwd[:M] = hist[hl - M:]
    iterate(fwd, fwd, ma_terms)
    res = [0.0] * (T + nF)                                                        # [5]
    res[:d] = ts[:d]
    res[d:d + hl - M] = hist[M:]                                                  # [6]
    res[T:] = fwd[M:]
    if d != 0:                                                                    # [7]
        dm = [[0.0] * T for _ in range(d + 1)]
        dm[0] = list(ts)
        for i in range(1, d + 1):
            dm[i][i:] = O.differences_of_order_d(np.asarray(dm[i - 1][i:]), 1).tolist()
        for i in range(d, hl - M):
            s = 0.0
            for r in range(d):
                s = s + dm[r][i - 1]
            res[i] = s + hist[M + i]
        prev = [dm[r][T - d + r] for r in range(d)]
        res[T + nF - (d + nF):] = O.inverse_differences_of_order_d(np.asarray(prev + fwd[M:]), d).tolist()
    return res[nF:]


def arimax_forecast_batch(series, x, p, d, q, xreg_max_lag, include_original_xreg, include_intercept, coef):
    """Forecasts of every row; x shared or per series; coef (K',) or (N, K'): (N, T)."""
    series = np.ascontiguousarray(series, dtype=np.float64)
    N = series.shape[0]
    coef = np.asarray(coef, dtype=np.float64)
    return np.array([arimax_forecast(series[i], _x_of(x, i), p, d, q, xreg_max_lag, include_original_xreg,
                                     include_intercept, coef[i] if coef.ndim > 1 else coef) for i in range(N)])
