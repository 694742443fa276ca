"""The CPU restatement (oracle/) against the reference's own known-answer tests and data files.

These are the only pins of the oracle to spark-ts itself (the JVM reference cannot run here).
Tolerances are the reference tests' own.
"""
import numpy as np
import pytest

import oracle as O
from conftest import GOLDEN
from jvm_random import MersenneTwister

DS1 = np.loadtxt(f"{GOLDEN}/ds1.csv")
DS2 = np.loadtxt(f"{GOLDEN}/ds2.csv")


def mt_gauss(seed, n):
    return np.array(MersenneTwister(seed).gaussians(n))


def test_compare_with_r_ds1():
    # ARIMASuite.scala:27-41 (+-0.05) and python test_ARIMA.py:20-25 (+-0.01)
    r = O.fit(DS1, 1, 0, 1)
    assert r["status"] == 0
    c, ar, ma = r["coef"]
    assert abs(ar - 0.3) < 0.01 and abs(ma - 0.7) < 0.01


def test_compare_with_r_user_init_path_dependent():
    # test_ARIMA.py:27-32: user init [0, 0.2, 1.0] -> ar 0.55 +- 0.01, ma 1.03 +- 0.01 (pins the optimizer path)
    r = O.fit(DS1, 1, 0, 1, user_init=[0.0, 0.2, 1.0])
    c, ar, ma = r["coef"]
    assert abs(ar - 0.55) < 0.01 and abs(ma - 1.03) < 0.01


def test_integrated_order_3_ds2():
    # ARIMASuite.scala:134-156: ARIMA(0,3,1) ma 0.2 +- 0.05 (R CSS: 0.2523)
    r = O.fit(DS2, 0, 3, 1)
    assert abs(r["coef"][1] - 0.2) < 0.05


@pytest.mark.parametrize("smear", [0, 1])
def test_sampled_212_refit(smear):
    # ARIMASuite.scala:43-56 (and test_ARIMA.py:34-46): refit within 0.1, intercept within 1
    model = [8.2, 0.2, 0.5, 0.3, 0.1]
    s = O.add_time_dependent_effects(mt_gauss(10, 1000), 2, 1, 2, 1, model)
    r = O.fit(s, 2, 1, 2, smear=smear)
    c, a1, a2, m1, m2 = r["coef"]
    assert abs(c - 8.2) < 1
    assert abs(a1 - 0.2) < 0.1 and abs(a2 - 0.5) < 0.1 and abs(m1 - 0.3) < 0.1 and abs(m2 - 0.1) < 0.1


def test_arima_equals_arma_on_differenced():
    # ARIMASuite.scala:76-97: exact equality of ARIMA(1,1,2) and ARMA(1,0,2) on the differenced sample
    s = O.add_time_dependent_effects(mt_gauss(10, 1000), 1, 1, 2, 0, [0.3, 0.7, 0.1])
    a = O.fit(s, 1, 1, 2, intercept=False)
    b = O.fit(O.differences_of_order_d(s, 1)[1:], 1, 0, 2, intercept=False)
    assert abs(a["coef"][0] - 0.3) < 0.05 and abs(a["coef"][1] - 0.7) < 0.05 and abs(a["coef"][2] - 0.1) < 0.05
    assert np.array_equal(a["coef"], b["coef"])


def test_add_remove_effects_roundtrip():
    # ARIMASuite.scala:99-112
    wn = mt_gauss(20, 100)
    coef = [8.3, 0.1, 0.2, 0.3]
    proc = O.add_time_dependent_effects(wn, 1, 1, 2, 1, coef)
    back = O.remove_time_dependent_effects(proc, 1, 1, 2, 1, coef)
    assert np.max(np.abs(wn - back)) < 1e-4


def test_arima000_mean_and_forecast():
    # ARIMASuite.scala:114-132
    s = mt_gauss(10, 100)
    r = O.fit(s, 0, 0, 0)
    mean = s.sum() / s.size
    assert abs(r["coef"][0] - mean) < 1e-4
    f = O.forecast(s, 0, 0, 0, 1, r["coef"], 10)
    assert np.all(np.abs(f[100:] - mean) < 1e-4)


def test_stationarity_invertibility_kats():
    # ARIMASuite.scala:158-179, test_ARIMA.py:48-64
    assert not O.is_stationary([0.2, 1.5], 1, 0, 1) and O.is_invertible([0.2, 1.5], 1, 0, 1)
    assert O.is_stationary([0.13, 1.8], 0, 1, 1) and not O.is_invertible([0.13, 1.8], 0, 1, 1)
    assert O.is_stationary([0.003359, 1.545, -0.5646], 2, 0, 1)
    assert O.is_stationary([-0.09341, 0.857361, -0.300821], 1, 1, 1)
    assert O.is_invertible([-0.09341, 0.857361, -0.300821], 1, 1, 1)


def test_find_roots_kats():
    # ARIMASuite.scala:213-223
    assert abs(abs(O.find_roots([1, -0.4])[0]) - 2.5) < 1e-12
    roots = sorted(np.round(np.abs(O.find_roots([1, 0.5, -0.3, 1.9, -3.0, 0.5])), 5))
    assert roots == sorted([0.77959, 0.55383, 0.77959, 1.12229, 5.29438])


def test_differencing_kats():
    # UnivariateTimeSeriesSuite.scala:114-158 (exact at lag, order-d round trip)
    s = mt_gauss(10, 100)
    d1 = O.differences_of_order_d(s, 1)
    assert d1[10] == s[10] - s[9] and d1[99] == s[99] - s[98] and d1[0] == s[0]
    d5 = O.differences_of_order_d(s, 5)
    assert np.max(np.abs(O.inverse_differences_of_order_d(d5, 5) - s)) < 1e-6
    d6 = O.differences_of_order_d(s, 6)
    once_more = O.differences_of_order_d(d5, 1)
    assert np.max(np.abs(d6[6:] - once_more[6:])) < 1e-6


def test_lag_matrix_layout_kat():
    # UnivariateTimeSeriesSuite.scala:30-38, exactly: lag([1..5], 2, true) = Matrices.dense(3, 3, [3,4,5,2,3,4,1,2,3])
    # and lag([1..5], 2, false) = Matrices.dense(3, 2, [2,3,4,1,2,3]) (column-major values)
    x = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    rows, cols, v = O.lag_matrix(x, 2, True)
    assert (rows, cols) == (3, 3) and v.tolist() == [3.0, 4.0, 5.0, 2.0, 3.0, 4.0, 1.0, 2.0, 3.0]
    rows, cols, v = O.lag_matrix(x, 2, False)
    assert (rows, cols) == (3, 2) and v.tolist() == [2.0, 3.0, 4.0, 1.0, 2.0, 3.0]
    # the AR design of Autoregression.fitModel is that matrix (the oracle's AR fit builds it with the same code): an
    # exact AR(2) recursion is recovered through the intercept-free OLS
    y = [1.0, 2.0]
    for _ in range(10):
        y.append(0.5 * y[-1] + 0.25 * y[-2])
    st, c, a = O.ar_fit(np.array(y), 2, no_intercept=True)
    assert st == 0 and np.allclose(a, [0.5, 0.25], atol=1e-12)


@pytest.mark.parametrize("coef", [[1.5, 0.2], [1.5, 0.2, 0.3]])
def test_autoregression_kats(coef):
    # AutoregressionSuite.scala:26-44: ARModel(c, phi).sample(5000, MT(10)), fit within 0.03 (c within .07/.15)
    noise = mt_gauss(10, 5000)
    p = len(coef) - 1
    ts = np.empty(5000)
    for i in range(5000):        # ARModel.addTimeDependentEffects (Autoregression.scala:75-87)
        v = coef[0] + noise[i]
        for j in range(p):
            if i - j - 1 >= 0:
                v += ts[i - j - 1] * coef[1 + j]
        ts[i] = v
    st, c, a = O.ar_fit(ts, p)
    assert st == 0
    assert abs(c - 1.5) < (0.07 if p == 1 else 0.15)
    assert np.all(np.abs(a - np.array(coef[1:])) < 0.03)


def test_fdlibm_log_is_within_one_ulp():
    rng = np.random.default_rng(1)
    xs = np.concatenate([rng.uniform(1e-3, 1e3, 2000), np.exp(rng.uniform(-700, 700, 2000)), [1.0, 2.0, 0.5]])
    for x in xs:
        a, b = O.log(x), np.log(x)
        assert abs(a - b) <= np.spacing(abs(b)) * 1.0 + 0.0
    assert O.log(1.0) == 0.0 and np.isneginf(O.log(0.0)) and np.isnan(O.log(-1.0))


def test_status_semantics():
    # NaN input -> NaN-absorbing objective -> TooManyEvaluations after 10000 counted evaluations
    s = np.full(120, np.nan)
    r = O.fit(s, 1, 0, 1)
    assert r["status"] == 1 and r["n_eval"] == 10000
    # constant series: AR(m) design has collinear columns -> SingularMatrixException
    assert O.fit(np.full(50, 3.0), 1, 1, 1)["status"] == 4
    # ARIMA(0,0,0) without intercept: OLS with zero columns -> NoDataException
    assert O.fit(np.arange(30.0), 0, 0, 0, intercept=False)["status"] == 6
    # unknown method after a successful HR init -> UnsupportedOperationException
    assert O.fit(DS1, 1, 0, 1, method=99)["status"] == 9


KPSS_R_V = [0.0187461709418264, -0.184252542069064, -1.37133054992251, -0.599167715783718,
            0.294545126567508, 0.389794300700167, -1.20807617542949, -0.363676017470862,
            -1.62667268170309, -0.256478394123992, 1.10177950308713, 0.755781508027337,
            -0.238233556018718, 0.98744470341339, 0.741390128383824, 0.0893472664958216,
            -0.954943856152377, -0.195150384667239, 0.92552126209408, 0.482978524836611]


def test_kpss_r_equivalence():
    # TimeSeriesStatisticalTestsSuite.scala:102-142 (R tseries::kpss.test on set.seed(10); rnorm(20)): Level 0.27596,
    # Trend 0.05092, within 1e-4
    st, c = O.kpss(KPSS_R_V, "c")
    st2, ct = O.kpss(KPSS_R_V, "ct")
    assert st == 0 and st2 == 0
    assert abs(c - 0.2759) < 1e-4 and abs(ct - 0.05092) < 1e-4
    # the OLS shape check: one regressor needs at least two rows (AbstractMultipleLinearRegression.validateSampleData)
    assert O.kpss([1.0], "c")[0] == 5 and O.kpss([], "c")[0] == 6


def _kpss_long_double(row):
    """kpsstest(ts, "c") by its formula (TimeSeriesStatisticalTests.scala:369-431) in long double, not by the
    reference's steps: residuals about the mean, the sum of the squared cumulative sums, the Bartlett-weighted
    autocovariances up to (3 sqrt(n) / 13).toInt, and n * n as a float (no Int product)."""
    y = np.asarray(row, dtype=np.longdouble)
    n = len(y)
    e = y - y.sum() / n
    s2 = (np.cumsum(e) ** 2).sum()
    lag = int(3 * np.sqrt(n) / 13)
    terms = np.longdouble(0)
    for i in range(1, lag + 1):
        terms += (e[i:] * e[:-i]).sum() * (1 - np.longdouble(i) / (lag + 1))
    long_run_variance = 2 * terms / n + (e * e).sum() / n
    return s2 / long_run_variance / (np.longdouble(n) * n)


# The restatement's worst relative difference from the long-double formula over the rows below is 1.53e-11 (T = 2, a
# random walk * 1e3 + 1e6: the mean's rounding against residuals of ~1e3; 1.4e-12 at most from T = 3 on). The bound is
# ten times that: room for another libm or long-double format, while a wrong lag or Bartlett weight moves the statistic
# by parts in a hundred.
KPSS_FORMULA_RTOL = 1.53e-10


@pytest.mark.parametrize("T", [2, 3, 18, 19, 75, 76, 300, 1024, 4096, 20448, 20449, 46340])
def test_kpss_matches_long_double_formula(T):
    rng = np.random.default_rng(7000 + T)
    rows = np.concatenate([rng.standard_normal((2, T)), np.cumsum(rng.standard_normal((2, T)), axis=1),
                           np.cumsum(rng.standard_normal((2, T)), axis=1) * 1e3 + 1e6])
    for i, row in enumerate(rows):
        st, stat = O.kpss(row, "c")
        ref = _kpss_long_double(row)
        assert st == 0 and np.isfinite(ref)
        rel = float(abs(stat - ref) / abs(ref))
        assert rel <= KPSS_FORMULA_RTOL, (T, i, stat, float(ref), rel)


def _autofit_kat_series():
    # ARIMASuite.scala:181-185: ARIMAModel(2, 0, 0, [2.5, 0.4, 0.3], true).sample(250, new MersenneTwister(10L))
    sampled = O.add_time_dependent_effects(mt_gauss(10, 250), 2, 0, 0, 1, [2.5, 0.4, 0.3])
    return sampled, O.inverse_differences_of_order_d(sampled, 5)


def test_autofit_kats():
    # ARIMASuite.scala:181-211
    sampled, high_i = _autofit_kat_series()
    assert O.autofit(high_i)["status"] == O.ST_NOT_STATIONARY          # Try(autoFit(highI)).isFailure
    r10 = O.autofit(high_i, max_d=10)                                   # Try(autoFit(highI, maxD = 10)).isSuccess
    assert r10["status"] == 0 and r10["order"][1] >= 1
    r = O.autofit(sampled, 5, 2, 5)
    assert r["status"] == 0
    p, d, q, I = r["order"]
    k = p + q + I
    fitted_aic = -2 * O.loglik_css(sampled, p, d, q, I, r["coef"][:k]) + 2 * k      # fitted.approxAIC(sampled)
    ji = O.fit(sampled, 0, d, 0, True)                                  # fitModel(0, fitted.d, 0, sampled)
    ji_aic = -2 * O.loglik_css(sampled, 0, d, 0, 1, ji["coef"]) + 2
    assert ji_aic > fitted_aic


def test_autofit_walk_quirks():
    # findBestARMAModel restated with its quirks (ARIMA.scala:310-375): the first round fits (0,0), (2,2), (1,0), (0,1)
    # with the d-dependent intercept; later rounds vary p and flip the intercept, never q; a candidate is fitted once
    sampled, _ = _autofit_kat_series()
    trace = []
    r = O.autofit(sampled, 5, 2, 5, trace=trace)
    assert trace[0] == [(0, 0, 1), (2, 2, 1), (1, 0, 1), (0, 1, 1)]
    q_first = {c[1] for c in trace[0]}
    for rnd in trace[1:]:
        assert len({c[1] for c in rnd}) == 1 and rnd[0][1] in q_first      # one q per later round
    assert r["n_fits"] == len({c for rnd in trace for c in rnd})
    # d = 2 (two unit roots): no intercept in the walk (addIntercept = d <= 1, :300)
    rw2 = O.inverse_differences_of_order_d(sampled, 2)
    tr2 = []
    r2 = O.autofit(rw2, 5, 2, 5, trace=tr2)
    assert r2["order"][1] == 2 and tr2[0][0] == (0, 0, 0)
    # maxQ = 0 / maxP = 0 bound only the neighbourhood, not the first candidates (:325-327, :369-370)
    tr3 = []
    O.autofit(sampled, 0, 2, 0, trace=tr3)
    assert tr3[0] == [(0, 0, 1), (2, 2, 1), (1, 0, 1), (0, 1, 1)] and all(c[0] == 0 and c[1] == 0 for rnd in tr3[1:]
                                                                          for c in rnd)


@pytest.mark.parametrize("name", ["autofit_kat_maxd2", "autofit_kat_maxd10", "autofit_mixed_T256_p2q1"])
def test_autofit_fixtures_match_the_oracle(name):
    # the committed autoFit vectors (tests/golden/make_golden_autofit.py) are the current restatement's outputs
    from conftest import load_case
    meta, arr = load_case(name)
    for i, row in enumerate(arr["series"]):
        r = O.autofit(row, meta["max_p"], meta["max_d"], meta["max_q"])
        assert r["status"] == arr["status"][i] and tuple(r["order"]) == tuple(arr["order"][i])
        assert r["n_fits"] == arr["n_fits"][i]
        assert np.array_equal(r["coef"], arr["coef"][i], equal_nan=True) and (r["aic"] == arr["aic"][i])


def test_bobyqa_similar_to_cgd_kat():
    # ARIMASuite.scala:58-74: ARIMAModel(2,1,2,[8.2,0.2,0.5,0.3,0.1]).sample(1000, MersenneTwister(10)) fitted with
    # css-bobyqa and css-cgd: intercepts within 1, the other coefficients within 0.1
    s = O.add_time_dependent_effects(mt_gauss(10, 1000), 2, 1, 2, 1, [8.2, 0.2, 0.5, 0.3, 0.1])
    b = O.fit(s, 2, 1, 2, method=1)
    c = O.fit(s, 2, 1, 2)
    assert b["status"] == 0 and c["status"] == 0 and b["n_grad"] == 0 and b["n_eval"] > 2 * 5 + 1
    assert abs(b["coef"][0] - c["coef"][0]) < 1
    assert np.all(np.abs(b["coef"][1:] - c["coef"][1:]) < 0.1)
    # BOBYQA maximises the same objective: it ends at least as high as the CG fit's loose stopping point here
    assert b["ll"] >= c["ll"]


def test_bobyqa_status_semantics():
    # BOBYQAOptimizer.setup: dimension >= 2 (NumberIsTooSmallException) -- after the Hannan-Rissanen init
    assert O.fit(DS1, 0, 0, 1, intercept=False, method=1)["status"] == 14
    assert O.fit(DS1, 0, 0, 0, intercept=False, method=1)["status"] == 6          # HR throws first (NoData)
    assert O.fit(DS1, 2, 0, 0, method=1)["status"] == 0                           # AR-only shortcut, no method
    r = O.fit(DS1, 1, 0, 1, method=1, user_init=[0.0, 0.2, 1.0])
    assert r["status"] == 0 and abs(r["coef"][1] - 0.3) < 0.05 and abs(r["coef"][2] - 0.7) < 0.05
