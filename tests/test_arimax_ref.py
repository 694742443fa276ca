"""The ARIMAX restatement (tests/arimax_ref.py) against the reference suite's six cases under both readings of the Breeze
overlap, its own invariants, and the conditions the device tests' inputs have to meet. No GPU."""
import numpy as np
import pytest

import arimax_cases as C
import arimax_ref as AX
import oracle as O
import regress_ref as R
import smallfit_ref as S

CASES = C.suite_cases()
IDS = [c["name"] for c in CASES]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).tolist()


def _ka(c):
    return int(c["include_intercept"]) + c["p"] + c["q"]


def _forecast(c, coef):
    _, _, ts_test, x_test = C.suite_data()[c["data"]]
    return AX.arimax_forecast(ts_test, x_test, c["p"], c["d"], c["q"], c["xreg_max_lag"], c["include_original_xreg"],
                              c["include_intercept"], coef)


def _check_suite_assertions(c, r):
    """What ARIMAXSuite asserts of a fitted model: coefficients.length, the forecast's length and its band."""
    _, _, ts_test, _ = C.suite_data()[c["data"]]
    assert len(r["coef"]) == c["num_coef"]
    f = _forecast(c, r["coef"])
    assert len(f) == len(ts_test)
    s = 0.0
    for v in ts_test:
        s += v
    avg = s / len(ts_test)
    tol = c["tolerance"] * (max(abs(v - avg) for v in ts_test) if c["tolerance_times_max_deviation"] else 1.0)
    assert all(abs(v - avg) <= tol for v in f), (c["name"], max(abs(v - avg) for v in f), tol)


# ---- the reference suite, under both readings -------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(6), ids=IDS)
def test_suite_under_the_shift_reading(idx):
    r = C.suite_fit(idx, 0)
    assert r["status"] == AX.ST_OK
    _check_suite_assertions(CASES[idx], r)


@pytest.mark.parametrize("idx", range(6), ids=IDS)
def test_suite_under_the_smear_reading(idx):
    """Five cases pass; "MAX(0,0,2) 1 true" runs to MaxEval, a TooManyEvaluationsException in the JVM -- and so does the
    plain ARIMA(0,0,2) fit from the same start, so the composition is not what fails."""
    c, r = CASES[idx], C.suite_fit(idx, 1)
    if c["name"] != "MAX(0,0,2) 1 true":
        assert r["status"] == AX.ST_OK
        _check_suite_assertions(c, r)
        return
    assert (r["status"], r["n_eval"]) == (S.ST_MAX_EVAL, 10000)
    assert np.all(np.isnan(r["coef"])) and len(r["coef"]) == c["num_coef"]
    ts = C.suite_data()[c["data"]][0]
    plain = O.fit(ts, c["p"], c["d"], c["q"], True, user_init=r["init"][:_ka(c)], smear=1)
    assert (plain["status"], plain["n_eval"]) == (S.ST_MAX_EVAL, 10000)


def test_suite_fits_that_do_not_depend_on_the_reading():
    # q <= 1: one lag row, both readings are the same copy
    for idx, c in enumerate(CASES):
        if c["q"] <= 1:
            a, b = C.suite_fit(idx, 0), C.suite_fit(idx, 1)
            assert _bits(a["coef"]) == _bits(b["coef"]) and a["n_eval"] == b["n_eval"]


def test_the_restart_period_is_the_full_coefficient_count():
    idx = IDS.index("MAX(0,0,2) 1 true")
    c, r = CASES[idx], C.suite_fit(idx, 0)
    ka = _ka(c)
    assert (len(r["coef"]), ka) == (11, 3)
    ts = C.suite_data()[c["data"]][0]
    plain = O.fit(ts, c["p"], c["d"], c["q"], True, user_init=r["init"][:ka], smear=0)     # period ka
    assert plain["status"] == AX.ST_OK and r["status"] == AX.ST_OK
    assert (r["n_eval"], plain["n_eval"]) == (598, 882)
    assert _bits(r["coef"][:ka]) != _bits(plain["coef"])


@pytest.mark.parametrize("smear", [0, 1])
def test_inert_coordinates_come_back_as_they_started(smear):
    seen = 0
    for idx, c in enumerate(CASES):
        r = C.suite_fit(idx, smear)
        if r["status"] == AX.ST_OK:
            assert _bits(r["coef"][_ka(c):]) == _bits(r["init"][_ka(c):]), c["name"]
            assert _bits(r["coef"][:_ka(c)]) != _bits(r["init"][:_ka(c)]), c["name"]
            seen += 1
    assert seen == 6 - smear
    for cfg in C.CONFIGS:
        p, d, q, L, orig, icpt, T, k = C.CONFIGS[cfg]
        r = C.batch_ref(cfg, smear)
        ok = r["status"] == AX.ST_OK
        ka = int(icpt) + p + q
        assert _bits(r["coef"][ok][:, ka:]) == _bits(r["init"][ok][:, ka:]), cfg


def test_no_intercept_layout():
    for name, Kp in (("ARIMAX(2,1,1) 1 true false - first data set", 8), ("ARIMAX(2,1,1) 1 true false", 12)):
        idx = IDS.index(name)
        c, r = CASES[idx], C.suite_fit(idx, 0)
        assert len(r["init"]) == len(r["coef"]) == Kp and not c["include_intercept"]
        # slot 0 starts at 0.0 and is an ACTIVE coordinate: the objective reads it as the first AR coefficient, the
        # true second AR coefficient as theta_1, and the true theta_1 (slot 3) is inert
        assert r["init"][0] == 0.0 and r["coef"][0] != 0.0
        assert _bits(r["coef"][3:]) == _bits(r["init"][3:])
        ts, x = C.suite_data()[c["data"]][:2]
        diffed = O.differences_of_order_d(np.asarray(ts, dtype=np.float64), 1)[1:]
        assert r["ll"] == O.loglik_css_arma(diffed, 2, 1, 0, r["coef"][:3])


# ---- the start point ----------------------------------------------------------------------------------------------
def test_start_point_composition():
    c = CASES[IDS.index("ARIMAX(1,1,1) 1 true true")]
    ts, x = C.suite_data()[c["data"]][:2]
    st, init = AX.arimax_init(ts, x, 1, 1, 1, 1)
    assert st == AX.ST_OK and len(init) == 11
    # the matrix is differenced as one vector: column c >= 1 starts with a difference against column c - 1
    dx = AX.difference_xreg_flat(x, 1)
    assert dx[0][0] == x[0][0] and dx[1][0] == x[1][0] - x[0][-1] and dx[1][1] == x[1][1] - x[1][0]
    # the regression runs on the UNDIFFERENCED series
    ast, ac, acoef = R.arx_fit(ts, dx, 1, 1, True, False)
    diffed = O.differences_of_order_d(np.asarray(ts, dtype=np.float64), 1)[1:]
    hst, hr = O.hannan_rissanen(diffed, 1, 1, True)
    assert (ast, hst) == (0, 0)
    assert _bits(init) == _bits([ac, acoef[0], hr[-1]] + list(acoef[1:]))


def test_gradient_composition_is_the_literal_gradient():
    rng = np.random.default_rng(8)
    y = rng.standard_normal(37)
    for p, q, I, extra in ((1, 1, 1, 4), (2, 1, 0, 5), (0, 2, 1, 2), (1, 2, 1, 9), (2, 0, 1, 3), (0, 3, 0, 4)):
        for smear in (0, 1):
            for trial in range(4):
                c = rng.uniform(-0.6, 0.6, 1 + p + q + extra).tolist()
                if trial == 2 and q:
                    c[I + p] = float("inf")                    # a non-finite MA coefficient: NaN everywhere
                if trial == 3:
                    c[0] = 1e200                               # sigma2 overflows: 0 * Inf in the inert columns
                fast, lit = AX.gradient(y, p, q, I, c, smear), AX.gradient_literal(y, p, q, I, c, smear)
                assert len(fast) == len(c)
                assert np.array_equal(np.isnan(fast), np.isnan(lit)), (p, q, I, smear, trial)
                keep = ~np.isnan(fast)
                assert _bits(np.asarray(fast)[keep]) == _bits(np.asarray(lit)[keep]), (p, q, I, smear, trial)
    # a finite point: the inert columns are -0.0 (0 * error summed, divided by -sigma2), never NaN
    g = AX.gradient(y, 1, 1, 1, [0.1, 0.2, 0.3, 7.0, -2.0], 1)
    assert g[3:] == [0.0, 0.0] and all(np.signbit(v) for v in g[3:])
    # sigma2 == 0: 0 / -0 is NaN
    assert np.isnan(AX.inert_gradient([0.0] * 9, 1, 0, 0, [0.0, 5.0], 1))


# ---- the forecast ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,d,q,icpt", [(1, 0, 1, True), (2, 1, 1, True), (1, 2, 2, True), (0, 1, 2, True),
                                        (2, 0, 0, True), (2, 1, 1, False)])
def test_forecast_is_arimas_when_the_xreg_weight_is_zero(p, d, q, icpt):
    rng = np.random.default_rng(p * 100 + d * 10 + q)
    T, nF, k, L = 40, 9, 3, 2
    ts = np.cumsum(rng.standard_normal(T)) + 4.0
    x = rng.standard_normal((nF, k))
    coef = rng.uniform(-0.5, 0.5, AX.num_coef(k, p, q, L)).tolist()
    coef[p + q + k] = 0.0
    got = AX.arimax_forecast(ts, C.x_columns(x), p, d, q, L, True, icpt, coef)
    # ARIMA's layout: the intercept first when there is one; ARIMAX reads offset 1 either way
    arima_coef = coef[:1 + p + q] if icpt else coef[1:1 + p + q]
    want = O.forecast(ts, p, d, q, icpt, arima_coef, nF)[nF:]
    assert len(got) == T and _bits(got) == _bits(want)
    coef[p + q + k] = 0.25
    assert _bits(AX.arimax_forecast(ts, C.x_columns(x), p, d, q, L, True, icpt, coef)) != _bits(want)


def test_forecast_reads_only_the_last_column():
    rng = np.random.default_rng(2)
    T, nF, k = 33, 12, 3
    ts = rng.standard_normal(T)
    x = rng.standard_normal((nF, k))
    for orig, L in ((True, 1), (False, 2), (True, 0)):
        coef = rng.uniform(-0.5, 0.5, AX.num_coef(k, 1, 1, L, orig))
        want = AX.arimax_forecast(ts, C.x_columns(x), 1, 1, 1, L, orig, True, coef)
        bad = x.copy()
        bad[:, :k - 1] = np.nan
        bad[3, 0] = np.inf
        assert _bits(AX.arimax_forecast(ts, C.x_columns(bad), 1, 1, 1, L, orig, True, coef)) == _bits(want)
        assert not np.any(np.isnan(want))
        other = x.copy()
        other[:, k - 1] *= 2.0                        # (a shift would vanish in the differencing)
        assert _bits(AX.arimax_forecast(ts, C.x_columns(other), 1, 1, 1, L, orig, True, coef)) != _bits(want)
        # and of the xreg coefficients only coefficient p + q + k
        c2 = coef.copy()
        c2[3:] = np.where(np.arange(3, len(coef)) == 1 + 1 + k, coef[3:], np.nan)
        assert _bits(AX.arimax_forecast(ts, C.x_columns(x), 1, 1, 1, L, orig, True, c2)) == _bits(want)
    # no predictor at all (L = 0 without the original columns): ARIMA's forecast, K' = 1 + p + q
    coef = [0.3, 0.4, -0.2]
    got = AX.arimax_forecast(ts, C.x_columns(x), 1, 0, 1, 0, False, True, coef)
    assert _bits(got) == _bits(O.forecast(ts, 1, 0, 1, True, coef, nF)[nF:])


def test_forecast_xreg_term_by_hand():
    # p = 1, q = 0, d = 0, one column, L = 1 with the original column: step i reads X[i - 1 + L], X = [0] ++ x, the
    # column's value at t -- times coefficient p + q + k = 2, the slot of its LAG (counter k - 1 = 0), never slot 3
    ts, x, c = [1.0, 2.0, 4.0], [[10.0, 20.0]], [0.5, 0.25, 7.0, 2.0]
    got = AX.arimax_forecast(ts, x, 1, 0, 0, 1, True, True, c)
    X = [0.0, 10.0, 20.0]
    ext = [0.5] + ts
    hist = [0.5 + ext[i - 1] * 0.25 + (X[i - 1 + 1] * 7.0 if i - 1 < 3 - 1 else 0.0) for i in range(1, 4)]
    assert hist == [0.5 + 0.125 + 70.0, 0.5 + 0.25 + 140.0, 0.5 + 0.5 + 0.0]
    fwd = [hist[-1]]
    for i in (1, 2):
        fwd.append(0.5 + fwd[-1] * 0.25 + (X[i - 1 + 1] * 7.0 if i - 1 < 2 else 0.0))
    assert got == (hist + fwd[1:])[2:]


@pytest.mark.parametrize("kw,why", [
    (dict(p=0, q=0), "max"), (dict(k=0), "division"), (dict(nF=44, L=3), "transpose"), (dict(nF=45, L=3), "transpose"),
    (dict(nF=0, L=2), "fewer"), (dict(nF=2, d=2, L=2), "fewer"), (dict(T=1, d=2), "shorter")])
def test_forecast_shapes_that_throw(kw, why):
    a = dict(T=40, k=2, nF=5, p=1, d=0, q=1, L=1)
    a.update(kw)
    with pytest.raises(ValueError, match=why):
        AX.forecast_check(a["T"], a["k"], a["nF"], a["p"], a["d"], a["q"], a["L"])
    if a["k"]:
        x = [[1.0] * a["nF"] for _ in range(a["k"])]
        with pytest.raises(ValueError):
            AX.arimax_forecast([1.0] * a["T"], x, a["p"], a["d"], a["q"], a["L"], True, True, [0.1] * 20)


def test_forecast_shapes_at_the_boundaries_are_legal():
    for T, nF, d, L in ((40, 43, 0, 3), (40, 2, 0, 3), (40, 3, 2, 2), (2, 2, 2, 1)):    # nF - L == T; R == L; T == d
        coef = [0.1] * AX.num_coef(1, 1, 1, L)
        assert len(AX.arimax_forecast([1.0] * T, [[2.0] * nF], 1, d, 1, L, True, True, coef)) == T


# ---- the device tests' inputs meet their conditions ---------------------------------------------------------------
@pytest.mark.parametrize("cfg", sorted(C.CONFIGS))
def test_device_batches_are_mostly_ok_fits(cfg):
    q = C.CONFIGS[cfg][2]
    for smear in ((0, 1) if q == 2 else (1,)):
        st = C.batch_ref(cfg, smear)["status"]
        assert len(st) == C.N_MAX == 130 and int((st == AX.ST_OK).sum()) >= 117, (cfg, smear, np.bincount(st))
    assert int((C.batch_ref("a", 1, True)["status"] == AX.ST_OK).sum()) >= 117
    if q == 2:                                               # the readings differ where there are two lag rows
        assert _bits(C.batch_ref(cfg, 0)["coef"]) != _bits(C.batch_ref(cfg, 1)["coef"])


def test_device_edge_inputs():
    _, _, ref = C.edge_batch()
    st = ref["status"]
    assert st[C.EDGE_LANES["ones-column"]] == st[C.EDGE_LANES["ones-column-2"]] == R.ST_SINGULAR
    i = C.EDGE_LANES["nan-series"]
    assert np.all(np.isnan(ref["coef"][i])) and ref["n_eval"][i] > 0          # the optimizer runs on NaNs
    healthy = np.delete(np.arange(len(st)), list(C.EDGE_LANES.values()))
    assert int((st[healthy] == AX.ST_OK).sum()) >= len(healthy) - 2
    whole = C.batch_ref("a", 1)
    assert _bits(ref["coef"][healthy]) == _bits(whole["coef"][healthy])
    for name, (shape, arx_st, hr_st) in C.SHORT_CASES.items():
        p, d, q, L, orig, icpt, T, k = shape
        y, x, ref = C.short_case(name)
        assert R.arx_fit(y[0], AX.difference_xreg_flat(C.x_columns(x[0]), d), p, L, orig, False)[0] == arx_st, name
        assert O.hannan_rissanen(O.differences_of_order_d(y[0], d)[d:], p, q, icpt)[0] == hr_st, name
        assert np.all(ref["status"] == (arx_st or hr_st)) and np.all(np.isnan(ref["coef"])), name
    p, d, q, L, orig, icpt, T, k = C.WIDE
    assert AX.num_coef(k, p, q, L, orig) == 41 and AX.num_coef(k, p + 1, q, L, orig) == 42
    assert np.all(C.wide_case()[2]["status"] != R.ST_SINGULAR)
    y, x, init, ref = C.user_init_case()
    assert int((ref["status"] == AX.ST_OK).sum()) >= 55 and _bits(ref["init"]) == _bits(init)
    assert _bits(ref["coef"]) != _bits(C.batch_ref("a", 1)["coef"][:65])


def test_device_forecast_inputs():
    shapes = C.forecast_shapes()
    assert len(shapes) == 94                                 # 96 less the two forecast_check refuses
    # the streaming kernel serves these, the workspace kernel those
    assert all(max(s[4]) <= 5 and s[2] <= 8 for s in shapes)
    for s in C.FC_WORKSPACE_SHAPES:
        assert max(s[4]) > 5 or s[2] > 8
        AX.forecast_check(s[0], s[5], C.n_future_of(s[1], s[0], s[3][1]), s[4][0], s[2], s[4][1], s[3][1])
        assert C.forecast_case(s)[3].shape == (C.FC_N, s[0])
    assert {s[0] for s in shapes} == set(C.FC_T) and {s[1] for s in shapes} == set(C.FC_NF)
    assert {s[2] for s in shapes} == set(C.FC_D) and {s[3] for s in shapes} == set(C.FC_FLAGS)
    assert {s[4] for s in shapes} == set(C.FC_ORDERS) and {s[5] for s in shapes} == {1, 2, 3}
    assert {(s[0], s[1], s[2]) for s in shapes} == {(T, r, d) for T in C.FC_T for r in C.FC_NF for d in C.FC_D}
    y, x, coef, ref = C.forecast_case(next(s for s in shapes if s[5] == 3 and s[3][0] and s[3][1] > 0))
    assert ref.shape == y.shape and np.any(np.isnan(x[::5, :, 0]))
    clean = np.where(np.isfinite(x), x, 0.0)
    s = shapes[[i for i, s in enumerate(shapes) if s[5] == 3 and s[3][0] and s[3][1] > 0][0]]
    again = AX.arimax_forecast_batch(y, C.x_columns(clean), s[4][0], s[2], s[4][1], s[3][1], s[3][0], s[3][2], coef)
    assert _bits(again[~np.isnan(ref)]) == _bits(ref[~np.isnan(ref)]) and np.array_equal(np.isnan(again), np.isnan(ref))
    assert not np.any(np.isnan(ref[:7])) and np.all(np.isnan(ref[9, -1:])) and not np.any(np.isnan(ref[7]))


def test_device_forecast_slice_inputs():
    T, nF, d, (orig, L, icpt), (p, q), k = C.SLICE_SHAPE
    assert d > 8 and nF > d                                  # the workspace kernel, with predictor rows to read
    AX.forecast_check(T, k, nF, p, d, q, L)
    assert C.forecast_ws(T, d, max(p, q), nF) == 7772
    y, x, coef, sl, ref = C.slice_case()
    N = C.SLICE_N
    assert sl == 17269 and sl < N < 2 * sl and C.SLICE_WINDOW <= N - sl
    assert ref.shape == (2 * C.SLICE_REF, T) and np.isfinite(ref).all()
    # rows a slice apart differ everywhere, in every array the second launch offsets
    for a in (y, x, coef):
        assert not np.any(a[sl:] == a[:N - sl])
    # and each offset shows on its own: the first row of the second slice with one array taken a slice earlier
    i, want = sl, ref[C.SLICE_REF]

    def fc(ts, xm, c):
        return np.array(AX.arimax_forecast(ts, C.x_columns(xm), p, d, q, L, orig, icpt, c))

    assert _bits(fc(y[i], x[i], coef[i])) == _bits(want)
    assert not np.any(fc(y[0], x[i], coef[i]) == want)
    assert _bits(fc(y[i], x[0], coef[i])) != _bits(want) and _bits(fc(y[i], x[i], coef[0])) != _bits(want)
