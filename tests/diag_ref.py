"""CPU restatement of the reference's residual diagnostics, in pure Python floats and plain loops (IEEE fp64 in the
reference's order; math.sqrt is correctly rounded), written from the reference's behaviour:

  autocorr   UnivariateTimeSeries.autocorr       (UnivariateTimeSeries.scala:70-96)
  dwtest     TimeSeriesStatisticalTests.dwtest   (TimeSeriesStatisticalTests.scala:251-262)
  lbtest     TimeSeriesStatisticalTests.lbtest   (:298-307), n * (n + 2) in 32-bit Int arithmetic
  chisq_upper_tail   1 - ChiSquaredDistribution(L).cumulativeProbability(stat), commons-math3 3.4.1

The device code (csrc/arima_diag.hip, csrc/arima_chisq.hpp) is held to this file bit for bit, except the p-value,
which goes through exp and log and is held to a tolerance. Nothing is special-cased: 0/0 is NaN as in the JVM.
"""
import ctypes
import math

NAN = float("nan")
INF = float("inf")


def _div(a, b):
    """JVM double division: x / 0 is +-Inf or NaN, never an exception."""
    if b == 0.0:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def _sqrt(x):
    if x != x or x < 0.0:
        return NAN
    return math.sqrt(x)


def breeze_mean(xs):
    """Breeze `mean` of a slice, as the left fold sum += x from 0.0, then sum / m. Unpinned reading:
    Breeze is not vendored by the reference; the other reading is the running-mean update. Flip it here and in
    dg_mean_step / dg_mean_finish (csrc/arima_diag.hip) together."""
    s = 0.0
    for x in xs:
        s += x
    return _div(s, float(len(xs)))


def autocorr(ts, num_lags):
    ts = [float(x) for x in ts]
    T = len(ts)
    out = []
    for i in range(1, num_lags + 1):
        m = T - i
        slice1, slice2 = ts[i:], ts[:m]
        mean1, mean2 = breeze_mean(slice1), breeze_mean(slice2)
        v1 = v2 = cov = 0.0
        for j in range(m):
            d1 = slice1[j] - mean1
            d2 = slice2[j] - mean2
            v1 += d1 * d1
            v2 += d2 * d2
            cov += d1 * d2
        out.append(_div(cov, _sqrt(v1) * _sqrt(v2)))
    return out


def dwtest(r):
    r = [float(x) for x in r]
    resids = r[0] * r[0]
    diffs = 0.0
    for i in range(1, len(r)):
        resids += r[i] * r[i]
        diff = r[i] - r[i - 1]
        diffs += diff * diff
    return _div(diffs, resids)


def int_n_n2(n):
    """n * (n + 2) as the JVM's 32-bit Int product: wraps for n >= 46340."""
    return ctypes.c_int32(ctypes.c_int32(n).value * ctypes.c_int32(n + 2).value).value


def lb_stat_from_acf(acf, n):
    s = 0.0
    for k, p in enumerate(acf):
        s += _div(p * p, float(n - k - 1))
    return float(int_n_n2(n)) * s


def lbtest(r, max_lag):
    stat = lb_stat_from_acf(autocorr(r, max_lag), len(r))
    return stat, chisq_upper_tail(max_lag, stat)


# ---- commons-math3 3.4.1: ChiSquaredDistribution -> GammaDistribution -> Gamma.regularizedGammaP / Q -----------------
_EPS = 1e-15
_HALF_LOG_PI = 0.5723649429247001
_HALF_LOG_2_PI = 0.9189385332046727
_LANCZOS_G = 607.0 / 128.0
_LANCZOS = [0.99999999999999709182, 57.156235665862923517, -59.597960355475491248, 14.136097974741747174,
            -0.49191381609762019978, .33994649984811888699e-4, .46523628927048575665e-4, -.98374475304879564677e-4,
            .15808870322491248884e-3, -.21026444172410488319e-3, .21743961811521264320e-3, -.16431810653676389022e-3,
            .84418223983852743293e-4, -.26190838401581408670e-4, .36899182659531622704e-5]
_IMAX = 2147483647


def log_gamma_half(L):
    """logGamma(L / 2). Up to 8 the library evaluates an NSWC polynomial; at the half-integers chi-squared asks for,
    Gamma has a closed form that is exact in fp64 up to 8, and that is what is evaluated (csrc/arima_chisq.hpp)."""
    a = 0.5 * L
    if a <= 8.0:
        prod = 1.0
        if L % 2 == 0:
            for i in range(2, L // 2):
                prod *= float(i)
            return math.log(prod)
        for j in range(1, (L - 1) // 2 + 1):
            prod *= float(j) - 0.5
        return _HALF_LOG_PI + math.log(prod)
    s = 0.0
    for i in range(14, 0, -1):
        s += _LANCZOS[i] / (a + i)
    s += _LANCZOS[0]
    tmp = a + _LANCZOS_G + .5
    return ((a + .5) * math.log(tmp)) - tmp + _HALF_LOG_2_PI + math.log(s / a)


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return INF


def _log(x):
    return -INF if x == 0.0 else math.log(x)


def _gamma_p_series(a, x, lg):
    n, an = 0.0, 1.0 / a
    s = an
    while abs(an / s) > _EPS and n < _IMAX and s < INF:
        n += 1.0
        an *= x / (a + n)
        s += an
    if math.isinf(s):
        return 1.0
    return _exp(-x + (a * _log(x)) - lg) * s


def _gamma_q_cf(a, x, lg):
    small = 1e-50
    h_prev = 1.0 - a + x
    if abs(h_prev) <= small:
        h_prev = small
    d_prev, c_prev, h_n = 0.0, h_prev, h_prev
    n = 1
    while n < _IMAX:
        an = ((2.0 * n) + 1.0) - a + x
        bn = n * (a - n)
        d_n = an + bn * d_prev
        if abs(d_n) <= small:
            d_n = small
        c_n = an + bn / c_prev
        if abs(c_n) <= small:
            c_n = small
        d_n = 1 / d_n
        delta = c_n * d_n
        h_n = h_prev * delta
        if math.isinf(h_n) or h_n != h_n:
            return NAN                               # the library throws; the batch reports NaN
        if abs(delta - 1.0) < _EPS:
            break
        d_prev, c_prev, h_prev = d_n, c_n, h_n
        n += 1
    return _exp(-x + (a * _log(x)) - lg) * (1.0 / h_n)


def chisq_upper_tail(L, stat):
    if stat != stat:
        return NAN
    if stat <= 0.0:
        return 1.0
    a, x = L / 2.0, stat / 2.0
    lg = log_gamma_half(L)
    if x >= a + 1.0:
        cdf = 1.0 - _gamma_q_cf(a, x, lg)
    else:
        cdf = _gamma_p_series(a, x, lg)
    return 1.0 - cdf


def diagnostics(rows, max_lag):
    """All four outputs for every row of `rows`, as lists: (acf rows, dw, lb_stat, lb_pvalue)."""
    acf, dw, st, pv = [], [], [], []
    for r in rows:
        a = autocorr(r, max_lag)
        s = lb_stat_from_acf(a, len(r))
        acf.append(a)
        dw.append(dwtest(r))
        st.append(s)
        pv.append(chisq_upper_tail(max_lag, s))
    return acf, dw, st, pv
