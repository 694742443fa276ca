"""CPU restatement of the reference's regression with AR(1) errors, in pure Python floats and plain loops (IEEE fp64
in the reference's order, no fused multiply-add), written from the reference's behaviour:

  cochrane_orcutt   RegressionARIMA.fitCochraneOrcutt (RegressionARIMA.scala:83-160)
  is_autocorrelated RegressionARIMA.isAutoCorrelated  (:171-176) over diag_ref.dwtest
  simple_slope      commons-math3 3.4.1 SimpleRegression(false): addData, getSlope
  dgemv_fit         Breeze DenseMatrix * DenseVector = F2J dgemv('N'), then + beta(0)

The regressions are regress_ref.ols / residuals (OLSMultipleLinearRegression with an intercept). The device code
(k_cochrane_orcutt, csrc/arima_regress.hip) is held to this file bit for bit. Nothing is special-cased: a NaN rho makes
NaN designs, the QR goes through with NaN coefficients, the NaN Durbin-Watson statistic ends the loop with status OK.

Two readings are unpinned, because the reference vendors neither commons-math3 nor netlib: the sums of
SimpleRegression (simple_slope) and the order of F2J dgemv (dgemv_fit). Flip them here and in k_cochrane_orcutt
together; the reference's own suite (tests/golden/regarima) holds both to its tolerances.

A regressor matrix is a list of k columns, each a sequence of T values (the column-major DenseMatrix(T, k)).
"""
from diag_ref import NAN, _div, dwtest
from regress_ref import ST_OK, ols, residuals

DW_MARGIN = 0.05
RHO_DIFF_THR = 0.001
DOUBLE_MIN_VALUE = 5e-324

# why a series left the loop (reason() below)
STOP_BEFORE_LOOP, STOP_DW, STOP_RHO, STOP_MAX_ITER = "before-loop", "dw", "rho", "max-iter"


def is_autocorrelated(u):
    """dw <= (2 - 0.05) || dw >= (2 + 0.05), the bounds as the reference's double expressions; NaN: False."""
    dw = dwtest(u)
    return dw <= (2 - DW_MARGIN) or dw >= (2 + DW_MARGIN)


def simple_slope(res):
    """SimpleRegression(false) over the pairs (res(i), res(i + 1)): sumXX += x * x; sumXY += x * y as left folds, then
    getSlope: NaN for n < 2 or |sumXX| < 10 * Double.MIN_VALUE, else sumXY / sumXX. Unpinned reading:
    flip it here and in k_cochrane_orcutt (csrc/arima_regress.hip) together."""
    n, sum_xx, sum_xy = 0, 0.0, 0.0
    for i in range(len(res) - 1):
        x, y = res[i], res[i + 1]
        sum_xx += x * x
        sum_xy += x * y
        n += 1
    if n < 2 or abs(sum_xx) < 10 * DOUBLE_MIN_VALUE:
        return NAN
    return _div(sum_xy, sum_xx)


def dgemv_fit(x, t, beta):
    """Row t of (regressors * beta.drop(1)) + beta(0): sum = 0.0; sum += beta(1 + c) * X(t, c) in column order, the
    intercept added last. Unpinned reading: flip it here and in k_cochrane_orcutt together."""
    s = 0.0
    for c in range(len(x)):
        s += beta[1 + c] * x[c][t]
    return s + beta[0]


def cochrane_orcutt(y, x, max_iter=10):
    """(status, beta[1 + k], rho, n_iter, tres_autocorrelated): regressionCoeff, arimaCoeff(0) and `iter` at exit. A
    series whose regression throws has that status, NaN beta and rho, and the iterations it had completed. The last
    value is isAutoCorrelated of the residuals the exit decision looked at (None for a failed series)."""
    if max_iter < 1:
        raise ValueError("max_iter < 1: the reference throws on every path")
    y = [float(v) for v in y]
    x = [[float(v) for v in col] for col in x]
    T, k = len(y), len(x)
    fail = [NAN] * (1 + k)
    rows = [[col[t] for col in x] for t in range(T)]
    st, beta = ols(y, rows, True, k)                                        # step 1
    if st != ST_OK:
        return st, fail, NAN, 0, None
    res = residuals(y, rows, beta, True)
    auto = is_autocorrelated(res)                                           # step 2
    finished = not auto
    rhos = [0.0] * max_iter
    it = 0
    while not finished:
        rho = simple_slope(res)                                             # (a)
        rhos[it] = rho
        ydash = [y[t] - y[t - 1] * rho for t in range(1, T)]                # (b)
        xdash = [[col[t] - col[t - 1] * rho for col in x] for t in range(1, T)]
        st, beta = ols(ydash, xdash, True, k)                               # (c)
        if st != ST_OK:
            return st, fail, NAN, it, None
        tres = residuals(ydash, xdash, beta, True)
        beta[0] = _div(beta[0], 1 - rho)                                    # (d)
        res = [y[t] - dgemv_fit(x, t, beta) for t in range(T)]              # (e)
        it += 1                                                             # (f)
        auto = is_autocorrelated(tres)                                      # (g)
        finished = (not auto) or it >= max_iter or (it >= 2 and abs(rhos[it - 1] - rhos[it - 2]) <= RHO_DIFF_THR)
    return ST_OK, beta, rhos[max(0, it - 1)], it, auto


def reason(fit, max_iter):
    """Which of (g)'s terms ended an OK fit, in the reference's order of evaluation."""
    st, _, _, it, auto = fit
    assert st == ST_OK
    if it == 0:
        return STOP_BEFORE_LOOP
    if not auto:
        return STOP_DW
    return STOP_MAX_ITER if it >= max_iter else STOP_RHO


def fit_batch(y, x, max_iter=10):
    """cochrane_orcutt over the rows of y (N, T) and the numpy array x, (N, T, k) or the shared (T, k): the four
    outputs of the device call as lists (coef, rho, n_iter, status), plus the fits themselves."""
    fits = [cochrane_orcutt(y[i], (x[i] if x.ndim == 3 else x).T.tolist(), max_iter) for i in range(len(y))]
    return [f[1] for f in fits], [f[2] for f in fits], [f[3] for f in fits], [f[0] for f in fits], fits
