"""tests/regress_ref.py, the CPU restatement the device regressions (csrc/arima_regress.hip) are held to: the
reference's own suites replayed with commons' MersenneTwister, bit identity of its QR with oracle.ols, and the
SecondMoment reading of calculateRSquared's total sum of squares."""
import numpy as np
import pytest

import oracle as O
import regress_ref as R
from jvm_random import MersenneTwister

# ---- AutoregressionXSuite (AutoregressionXSuite.scala:25-134), MersenneTwister(10) ----------------------------------
N_ROWS, N_COLS = 1000, 2
SUITE_TOL = 1e-4


@pytest.fixture(scope="module")
def arx_suite():
    """The suite's X (drawn row by row), then its intercept; x as columns for regress_ref."""
    rand = MersenneTwister(10)
    X = [[rand.next_gaussian() for _ in range(N_COLS)] for _ in range(N_ROWS)]
    intercept = rand.next_gaussian() * 10
    return X, [[row[c] for row in X] for c in range(N_COLS)], intercept


def _dot(row, coeffs):
    s = 0.0
    for b, v in zip(row, coeffs):
        s += b * v
    return s


def _scan(raw, coeff):
    """rawY.scanLeft(0.0) { (prior, curr) => curr + prior * coeff }.tail"""
    out, prior = [], 0.0
    for curr in raw:
        prior = curr + prior * coeff
        out.append(prior)
    return out


def _lagged(X, lag):
    """Lag.lagMatTrimBoth(X, lag): per column its lags 1 .. lag, columns concatenated."""
    return [[X[r - l][c] for c in range(N_COLS) for l in range(1, lag + 1)] for r in range(lag, len(X))]


def _suite_case(name, X, intercept):
    """(y, yMaxLag, xMaxLag, includeOriginalX, expected coefficients) of one of the suite's five fits."""
    if name == "1-0-true":
        return _scan([_dot(r, (0.8, 0.2)) + intercept for r in X], 0.4), 1, 0, True, [0.4, 0.8, 0.2]
    if name == "0-1-false":
        return [0.0] + [_dot(r, (0.4, 0.15)) + intercept for r in _lagged(X, 1)], 0, 1, False, [0.4, 0.15]
    if name == "0-0-true":
        return [_dot(r, (0.8, 0.2)) + intercept for r in X], 0, 0, True, [0.8, 0.2]
    if name == "0-2-true":
        lag = [_dot(r, (0.4, 0.15, 0.2, 0.7)) for r in _lagged(X, 2)]
        normal = [_dot(r, (0.3, 0.5)) for r in X][2:]
        return ([0.0, 0.0] + [l + n + intercept for l, n in zip(lag, normal)], 0, 2, True,
                [0.4, 0.15, 0.2, 0.7, 0.3, 0.5])
    assert name == "1-1-false"
    raw = [_dot(r, (0.8, 0.2)) + intercept for r in _lagged(X, 1)]
    return [0.0] + _scan(raw, 0.4), 1, 1, False, [0.4, 0.8, 0.2]


ARX_SUITE_CASES = ["1-0-true", "0-1-false", "0-0-true", "0-2-true", "1-1-false"]


@pytest.mark.parametrize("name", ARX_SUITE_CASES)
def test_arx_suite_fits(arx_suite, name):
    X, xcols, intercept = arx_suite
    y, yl, xl, orig, want = _suite_case(name, X, intercept)
    st, c, coef = R.arx_fit(y, xcols, yl, xl, orig)
    assert st == R.ST_OK
    assert abs(c - intercept) <= SUITE_TOL, (c, intercept)
    assert len(coef) == len(want)
    for got, exp in zip(coef, want):
        assert abs(got - exp) <= SUITE_TOL, (coef, want)


PREDICT_COEFFS = [-1.136026484226831e-08, 8.637677568908233e-07, 15238.143039368977, -7.993535860373772e-09,
                  -5.198597570089805e-07, 1.5691547009557947e-08, 7.409621376205488e-08]
PREDICT_X = [465, 1, 0.006562479, 24, 1, 0, 51]


def test_arx_suite_predict():
    out = R.arx_predict([100.0], [[v] for v in PREDICT_X], 0, PREDICT_COEFFS, 0, 0, True)
    assert len(out) == 1 and abs(out[0] - 100.0) <= SUITE_TOL, out


# ---- TimeSeriesStatisticalTestsSuite "breusch-godfrey" / "breusch-pagan" (:25-84), MersenneTwister(5) ---------------
def _first_stage_residuals(y, x):
    """OLSMultipleLinearRegression.newSampleData(y, x.map(Array(_))).estimateResiduals()"""
    rows = [[v] for v in x]
    st, beta = R.ols(y, rows, True)
    assert st == R.ST_OK
    return R.residuals(y, rows, beta)


def bg_suite():
    """(x, resids1, resids2) of the breusch-godfrey suite."""
    rand = MersenneTwister(5)
    x = [1.0, -1.0] * 50
    y1 = [v + 1 + rand.next_gaussian() for v in x]
    y2, prior = [], 0.0
    for curr in y1:                                   # scanLeft(0.0) { (prior, curr) => prior * coef + curr }.tail
        prior = prior * 0.5 + curr
        y2.append(prior)
    return x, _first_stage_residuals(y1, x), _first_stage_residuals(y2, x)


def bp_suite():
    """(x, resids1, resids2) of the breusch-pagan suite."""
    rand = MersenneTwister(5)
    x = [-1.0, 1.0] * 50
    err1 = [rand.next_gaussian() for _ in range(100)]
    err2 = [e * 2 if i % 2 == 0 else e for i, e in enumerate(err1)]
    y1 = [xi + ei + 1 for xi, ei in zip(x, err1)]
    y2 = [xi + ei + 1 for xi, ei in zip(x, err2)]
    return x, _first_stage_residuals(y1, x), _first_stage_residuals(y2, x)


def test_breusch_godfrey_suite():
    x, resids1, resids2 = bg_suite()
    for lag in (1, 4):
        st, _, p = R.bgtest(resids1, [x], lag)
        assert st == R.ST_OK and p > 0.05, (lag, p)
        st, _, p = R.bgtest(resids2, [x], lag)
        assert st == R.ST_OK and p < 0.05, (lag, p)


def test_breusch_pagan_suite():
    x, resids1, resids2 = bp_suite()
    st, _, p = R.bptest(resids1, [x])
    assert st == R.ST_OK and p > 0.05, p
    st, _, p = R.bptest(resids2, [x])
    assert st == R.ST_OK and p < 0.05, p


# ---- the QR against the C restatement ----------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("C", [1, 2, 5, 13])
def test_ols_bit_identical_to_oracle(C, intercept):
    rng = np.random.default_rng(100 * C + int(intercept))
    ncx = C - 1 if intercept else C
    for rows in (C, C + 1, 40):
        X = rng.standard_normal((rows, ncx))
        Y = rng.standard_normal(rows)
        st, beta = R.ols(list(Y), X.tolist(), intercept, ncx)
        if ncx == 0:                                  # oracle.ols infers the column count from X's shape
            ost, obeta = O.ols(Y, np.empty((rows, 0)), intercept)
        else:
            ost, obeta = O.ols(Y, X, intercept)
        assert st == ost, (rows, st, ost)
        if st == R.ST_OK:
            assert np.array_equal(_bits(beta), _bits(obeta)), (rows, beta, obeta)
        else:
            assert beta is None


def test_ols_singular_and_not_enough_data():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((12, 3))
    X[:, 1] = 0.0                                     # an all-zero column: its rDiag is exactly 0
    Y = rng.standard_normal(12)
    assert R.ols(list(Y), X.tolist(), True)[0] == O.ols(Y, X, True)[0] == R.ST_SINGULAR
    X = rng.standard_normal((4, 4))                   # R = K
    Y = rng.standard_normal(4)
    assert R.ols(list(Y), X.tolist(), True)[0] == O.ols(Y, X, True)[0] == R.ST_NOT_ENOUGH_DATA
    assert R.ols([], [], True, 2)[0] == R.ST_NO_DATA


@pytest.mark.parametrize("no_intercept", [False, True])
@pytest.mark.parametrize("p", [1, 2, 5])
def test_arx_without_x_is_the_ar_fit(p, no_intercept):
    rng = np.random.default_rng(p)
    for T in (p, 2 * p, 2 * p + 1, 40):               # NO_DATA, NOT_ENOUGH_DATA (or the smallest shape), legal
        ts = np.cumsum(rng.standard_normal(T))
        st, c, coef = R.arx_fit(list(ts), [], p, 0, False, no_intercept)
        ost, oc, ocoef = O.ar_fit(ts, p, no_intercept)
        assert st == ost, (T, st, ost)
        if st == R.ST_OK:
            assert np.array_equal(_bits([c] + coef), _bits([oc] + list(ocoef)))
    assert R.arx_fit([1.0], [], 2, 0, False)[0] == O.ar_fit(np.array([1.0]), 2)[0] == R.ST_SERIES_TOO_SHORT


# ---- the SecondMoment reading -------------------------------------------------------------------------------------
# the largest relative difference between SecondMoment and the two-pass sum over the cases below, as this test prints
# it
SECOND_MOMENT_REL = 1.423e-15


def test_second_moment_against_two_pass():
    rng = np.random.default_rng(57)
    worst = 0.0
    for n in (2, 3, 10, 100, 1000):
        for scale, shift in ((1.0, 0.0), (1.0, 3.0), (10.0, -25.0), (0.01, 0.02)):
            ys = list(rng.standard_normal(n) * scale + shift)
            mean = sum(ys) / n
            two_pass = 0.0
            for y in ys:
                two_pass += (y - mean) * (y - mean)
            worst = max(worst, abs(R.second_moment(ys) - two_pass) / two_pass)
    print(f"SecondMoment vs two-pass: largest relative difference {worst:.3e}")
    assert worst <= 16 * SECOND_MOMENT_REL
