"""CPU restatement of the reference's regressions over a design matrix, in pure Python floats and plain loops (IEEE
fp64 in the reference's order, no fused multiply-add; math.sqrt is correctly rounded), written from the reference's
behaviour:

  arx_design / arx_fit / arx_predict   AutoregressionX.fitModel, ARXModel.predict (AutoregressionX.scala:48-130,
                                       Lag.scala:33-118)
  bg_design / bgtest                   TimeSeriesStatisticalTests.bgtest (TimeSeriesStatisticalTests.scala:276-288)
  bp_design / bptest                   TimeSeriesStatisticalTests.bptest (:320-329)
  ols                                  commons-math3 3.4.1 OLSMultipleLinearRegression: QRDecomposition (threshold 0)
                                       and its Solver, with the ARIMA_ST_* codes of its
                                       exceptions
  r_squared, second_moment             OLSMultipleLinearRegression.calculateRSquared

The device code (csrc/arima_regress.hip) is held to this file bit for bit, except the p-values, which go through exp
and log (diag_ref.chisq_upper_tail) and are held to a tolerance. Nothing is special-cased.

A regressor matrix is a list of k columns, each a sequence of T values (the column-major DenseMatrix(T, k)).
"""
from diag_ref import NAN, _div, _sqrt, chisq_upper_tail

ST_OK = 0
ST_SINGULAR = 4
ST_NOT_ENOUGH_DATA = 5
ST_NO_DATA = 6
ST_SERIES_TOO_SHORT = 10


def _cols(x):
    return [[float(v) for v in col] for col in x]


def arx_num_coef(k, y_max_lag, x_max_lag, include_original_x):
    return y_max_lag + k * x_max_lag + (k if include_original_x else 0)


def arx_design(y, x, y_max_lag, x_max_lag, include_original_x=True):
    """assemblePredictors and trimY: (rows R x K, response R), or None when R = T - maxLag < 0. Row r is time
    t = r + maxLag: y(t-1) .. y(t-yMaxLag), then per x column x_c(t-1) .. x_c(t-xMaxLag), then x_0(t) .. x_{k-1}(t)."""
    y, x = [float(v) for v in y], _cols(x)
    m = max(y_max_lag, x_max_lag)
    R = len(y) - m
    if R < 0:
        return None
    rows = []
    for r in range(R):
        t = r + m
        row = [y[t - l] for l in range(1, y_max_lag + 1)]
        for col in x:
            row += [col[t - l] for l in range(1, x_max_lag + 1)]
        if include_original_x:
            row += [col[t] for col in x]
        rows.append(row)
    return rows, y[m:]


def bg_design(u, factors, max_lag):
    """bgtest's auxiliary regression: rows t = maxLag .. T-1 of [factors(t, .), u(t-1) .. u(t-maxLag)], response
    u(t); None when T - maxLag < 0."""
    u, f = [float(v) for v in u], _cols(factors)
    R = len(u) - max_lag
    if R < 0:
        return None
    rows = [[col[t] for col in f] + [u[t - l] for l in range(1, max_lag + 1)] for t in range(max_lag, len(u))]
    return rows, u[max_lag:]


def bp_design(u, factors):
    """bptest's auxiliary regression: T rows of factors(t, .), response u(t) * u(t)."""
    u, f = [float(v) for v in u], _cols(factors)
    return [[col[t] for col in f] for t in range(len(u))], [v * v for v in u]


def ols(Y, X, intercept, ncx=None):
    """OLSMultipleLinearRegression.newSampleData + estimateRegressionParameters over the rows X (R x ncx, no ones
    column) and the response Y: (status, beta), beta = [intercept?, columns ...], None unless status is OK. ncx: the
    column count, needed only when there are no rows."""
    rows = len(Y)
    if ncx is None:
        ncx = len(X[0]) if X else 0
    if rows <= 0:                                     # validateSampleData
        return ST_NO_DATA, None
    if ncx + 1 > rows:
        return ST_NOT_ENOUGH_DATA, None
    if not intercept and ncx == 0:                    # Array2DRowRealMatrix rejects zero columns
        return ST_NO_DATA, None
    cols = ncx + (1 if intercept else 0)
    # qrt[c][r]: the transposed design, the ones column first
    qrt = ([[1.0] * rows] if intercept else []) + [[float(X[r][c]) for r in range(rows)] for c in range(ncx)]
    rdiag = [0.0] * cols
    for minor in range(cols):                         # performHouseholderReflection
        qm = qrt[minor]
        norm = 0.0
        for row in range(minor, rows):
            norm = norm + qm[row] * qm[row]
        a = -_sqrt(norm) if qm[minor] > 0 else _sqrt(norm)
        rdiag[minor] = a
        if a != 0.0:
            qm[minor] = qm[minor] - a
            for col in range(minor + 1, cols):
                qc = qrt[col]
                alpha = 0.0
                for row in range(minor, rows):
                    alpha = alpha - qc[row] * qm[row]
                alpha = _div(alpha, a * qm[minor])
                for row in range(minor, rows):
                    qc[row] = qc[row] - alpha * qm[row]
    for i in range(cols):                             # Solver.isNonSingular at threshold 0
        if abs(rdiag[i]) <= 0.0:
            return ST_SINGULAR, None
    yv = [float(v) for v in Y]
    for minor in range(cols):                         # Solver.solve: Q^T y ...
        qm = qrt[minor]
        dot = 0.0
        for row in range(minor, rows):
            dot = dot + yv[row] * qm[row]
        dot = _div(dot, rdiag[minor] * qm[minor])
        for row in range(minor, rows):
            yv[row] = yv[row] + dot * qm[row]
    beta = [0.0] * cols
    for row in range(cols - 1, -1, -1):               # ... then R x = y
        yv[row] = _div(yv[row], rdiag[row])
        y_row = yv[row]
        beta[row] = y_row
        qr = qrt[row]
        for i in range(row):
            yv[i] = yv[i] - y_row * qr[i]
    return ST_OK, beta


def residuals(Y, X, beta, intercept=True):
    """estimateResiduals: y - X b, each fitted value the left fold sum = 0; sum += X[r][i] * b[i] over all columns, the
    ones column included (Array2DRowRealMatrix.operate)."""
    out = []
    for r in range(len(Y)):
        s = 0.0
        row = ([1.0] if intercept else []) + list(X[r])
        for i in range(len(row)):
            s += row[i] * beta[i]
        out.append(float(Y[r]) - s)
    return out


def second_moment(ys):
    """commons-math3 3.4.1 SecondMoment.evaluate: the running update n++; dev = y - m1; nDev = dev / n; m1 += nDev;
    m2 += ((double) n - 1) * dev * nDev, associated left to right. Unpinned reading: commons is not
    vendored by the reference; flip it here and in rg_second_moment (csrc/arima_regress.hip) together."""
    n, m1, m2 = 0, 0.0, 0.0
    for y in ys:
        n += 1
        dev = float(y) - m1
        n_dev = dev / float(n)
        m1 += n_dev
        m2 += (float(n) - 1.0) * dev * n_dev
    return m2


def r_squared(Y, X, beta):
    """calculateRSquared of a regression with an intercept: 1 - RSS / TSS, RSS the left fold of res * res
    (ArrayRealVector.dotProduct), TSS SecondMoment.evaluate(y)."""
    rss = 0.0
    for res in residuals(Y, X, beta, True):
        rss += res * res
    return 1.0 - _div(rss, second_moment(Y))


def arx_fit(y, x, y_max_lag, x_max_lag, include_original_x=True, no_intercept=False):
    """AutoregressionX.fitModel: (status, c, coefficients); c and the K coefficients are NaN unless status is OK."""
    K = arx_num_coef(len(x), y_max_lag, x_max_lag, include_original_x)
    d = arx_design(y, x, y_max_lag, x_max_lag, include_original_x)
    if d is None:
        return ST_SERIES_TOO_SHORT, NAN, [NAN] * K
    st, beta = ols(d[1], d[0], not no_intercept, K)
    if st != ST_OK:
        return st, NAN, [NAN] * K
    return (st, 0.0, beta) if no_intercept else (st, beta[0], beta[1:])


def arx_predict(y, x, c, coefficients, y_max_lag, x_max_lag, includes_original_x=True):
    """ARXModel.predict: results(r) = c, then += value * coefficients(col) in column order."""
    rows, _ = arx_design(y, x, y_max_lag, x_max_lag, includes_original_x)
    out = []
    for row in rows:
        s = float(c)
        for i, v in enumerate(row):
            s += v * float(coefficients[i])
        out.append(s)
    return out


def _test(d, n_obs, ncx, df):
    if d is None:
        return ST_SERIES_TOO_SHORT, NAN, NAN
    st, beta = ols(d[1], d[0], True, ncx)
    if st != ST_OK:
        return st, NAN, NAN
    stat = float(n_obs) * r_squared(d[1], d[0], beta)
    return st, stat, chisq_upper_tail(df, stat)


def bgtest(u, factors, max_lag):
    """(status, statistic, p-value): nObs * R^2 of the auxiliary regression against chi-squared(maxLag)."""
    return _test(bg_design(u, factors, max_lag), len(u) - max_lag, len(factors) + max_lag, max_lag)


def bptest(u, factors):
    """(status, statistic, p-value): T * R^2 of u^2 on the factors against chi-squared(k)."""
    return _test(bp_design(u, factors), len(u), len(factors), len(factors))
