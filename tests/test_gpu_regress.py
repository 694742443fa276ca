"""Batched AutoregressionX fits and predictions, bgtest and bptest on the device (csrc/arima_regress.hip) against the
CPU restatement tests/regress_ref.py: coefficients, predictions and the test statistics bit for bit (NaNs in the same
places), the statuses equal, the p-values to P_TOL."""
import numpy as np
import pytest

import regress_ref as R
import sparkts_amd._lib as L
from test_gpu_diag import P_TOL, _p_close, _same
from test_regress_ref import ARX_SUITE_CASES, PREDICT_COEFFS, PREDICT_X, SUITE_TOL, _suite_case, bg_suite, bp_suite
from test_regress_ref import arx_suite  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

T = 40
NMAX = 130
# (yMaxLag, xMaxLag, k, includeOriginalX, noIntercept); (3, 2, 3, T, F) has C = 13 columns
CONFIGS = [(1, 0, 2, True, False), (0, 1, 2, False, False), (0, 0, 2, True, False), (0, 2, 2, True, False),
           (1, 1, 2, False, False), (3, 2, 3, True, False), (2, 0, 1, True, True), (2, 0, 0, False, False)]
SENT = -7.0


def _ref_fit(y, x, yl, xl, orig, noint):
    """regress_ref over the rows of y (N, T) and x (N, T, k): (coef N x (1 + K), status N)."""
    coef, status = [], []
    for i in range(len(y)):
        st, c, cf = R.arx_fit(y[i], x[i].T, yl, xl, orig, noint)
        coef.append([c] + list(cf))
        status.append(st)
    return np.array(coef).reshape(len(y), -1), np.array(status, dtype=np.int32)


def _ref_predict(y, x, coef, yl, xl, orig):
    return np.array([R.arx_predict(y[i], x[i].T, coef[i, 0], coef[i, 1:], yl, xl, orig) for i in range(len(y))])


_ARX = {}


def _arx_case(cfg):
    """One batch of NMAX series per configuration and its restated fits and predictions, computed once; a smaller N
    is its leading rows (every series is its own computation)."""
    if cfg not in _ARX:
        yl, xl, k, orig, noint = cfg
        rng = np.random.default_rng(1000 + CONFIGS.index(cfg))
        x = rng.standard_normal((NMAX, T, k))
        y = np.cumsum(rng.standard_normal((NMAX, T)), axis=1) * 0.3 + x.sum(axis=2) + 2.0
        coef, status = _ref_fit(y, x, yl, xl, orig, noint)
        _ARX[cfg] = y, x, coef, status, _ref_predict(y, x, coef, yl, xl, orig)
    return _ARX[cfg]


# ---- 1. fit and predict, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, NMAX])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_arx_fit_and_predict_bit_parity(engine, cfg, N):
    yl, xl, k, orig, noint = cfg
    y, x, coef, status, pred = (a[:N] for a in _arx_case(cfg))
    assert np.all(status == R.ST_OK)
    got = engine.arx_fit(y, x, yl, xl, orig, noint)
    assert np.array_equal(got["status"], status)
    assert _same(got["coef"], coef), np.nanmax(np.abs(got["coef"] - coef))
    if noint:
        assert np.all(got["coef"][:, 0] == 0.0)
    assert _same(engine.arx_predict(y, x, yl, xl, orig, got["coef"]), pred)


def test_arx_shared_x_equals_copies(engine):
    yl, xl, k, orig, noint = CONFIGS[5]
    y = _arx_case(CONFIGS[5])[0]
    x = np.random.default_rng(5).standard_normal((T, k))
    per = np.ascontiguousarray(np.broadcast_to(x, (NMAX, T, k)))
    a, b = engine.arx_fit(y, x, yl, xl, orig, noint), engine.arx_fit(y, per, yl, xl, orig, noint)
    assert np.array_equal(a["status"], b["status"]) and _same(a["coef"], b["coef"])
    coef, status = _ref_fit(y[:3], per[:3], yl, xl, orig, noint)
    assert _same(a["coef"][:3], coef) and np.array_equal(a["status"][:3], status)
    assert _same(engine.arx_predict(y, x, yl, xl, orig, a["coef"]), engine.arx_predict(y, per, yl, xl, orig, a["coef"]))
    f = np.random.default_rng(6).standard_normal((T, 2))
    fper = np.ascontiguousarray(np.broadcast_to(f, (NMAX, T, 2)))
    for a, b in ((engine.bgtest(y, f, 2), engine.bgtest(y, fper, 2)), (engine.bptest(y, f), engine.bptest(y, fper))):
        assert _same(a["stat"], b["stat"]) and _same(a["pvalue"], b["pvalue"])
        assert np.array_equal(a["status"], b["status"])


@pytest.mark.parametrize("p", [1, 2, 5])
def test_arx_without_x_is_the_ar_fit(engine, p):
    y = _arx_case(CONFIGS[0])[0][:65]
    got = engine.arx_fit(y, None, p, 0, False, False)
    ar = engine.fit_batch(y, p, 0, 0, True)
    assert np.array_equal(got["status"], ar["status"]) and _same(got["coef"], ar["coef"])
    assert _same(engine.arx_fit(y, np.empty((65, T, 0)), p, 0, True, False)["coef"], ar["coef"])


# ---- 2. edges: the reference's status, NaN outputs, untouched neighbours ------------------------------------------
def _check_against_ref(engine, y, x, yl, xl, orig, noint, what):
    coef, status = _ref_fit(y, x, yl, xl, orig, noint)
    got = engine.arx_fit(y, x, yl, xl, orig, noint)
    assert np.array_equal(got["status"], status), (what, got["status"], status)
    assert _same(got["coef"], coef), what
    assert np.all(np.isnan(got["coef"][status != R.ST_OK])), what
    return status


@pytest.mark.parametrize("Tn,yl,xl,want", [(0, 0, 0, R.ST_NO_DATA), (0, 1, 0, R.ST_SERIES_TOO_SHORT),
                                           (2, 2, 1, R.ST_NO_DATA), (1, 0, 2, R.ST_SERIES_TOO_SHORT),
                                           (8, 2, 1, R.ST_NOT_ENOUGH_DATA),       # R = 6 = K
                                           (9, 2, 1, R.ST_OK)])                   # R = 7 = K + 1, the smallest
def test_arx_shape_edges(engine, Tn, yl, xl, want):
    rng = np.random.default_rng(Tn)
    y, x = rng.standard_normal((66, Tn)), rng.standard_normal((66, Tn, 2))
    status = _check_against_ref(engine, y, x, yl, xl, True, False, (Tn, yl, xl))     # K = yl + 2 xl + 2
    assert np.all(status == want)


def test_arx_zero_column_and_nan_leave_neighbours_alone(engine):
    cfg = CONFIGS[3]
    yl, xl, k, orig, noint = cfg
    y, x, coef, status, _ = (a[:70].copy() for a in _arx_case(cfg))
    x[5, :, 1] = 0.0                                   # SINGULAR
    x[64, :, 0] = 0.0
    y[7, 11] = np.nan                                  # the JVM goes on: status OK, NaN coefficients
    x[66, 3, 1] = np.nan
    st = _check_against_ref(engine, y, x, yl, xl, orig, noint, "zero column / NaN")
    assert st[5] == st[64] == R.ST_SINGULAR and st[7] == st[66] == R.ST_OK
    got = engine.arx_fit(y, x, yl, xl, orig, noint)
    touched = np.zeros(70, dtype=bool)
    touched[[5, 7, 64, 66]] = True
    assert np.all(np.isnan(got["coef"][touched]))
    assert _same(got["coef"][~touched], coef[~touched])


# ---- 3. bgtest and bptest -------------------------------------------------------------------------------------
def _check_test(got, ref, what):
    st = np.array([r[0] for r in ref], dtype=np.int32)
    assert np.array_equal(got["status"], st), (what, got["status"], st)
    assert _same(got["stat"], [r[1] for r in ref]), what
    assert _p_close(got["pvalue"], [r[2] for r in ref]), (what, P_TOL)
    return st


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("max_lag", [1, 4])
def test_bgtest_bit_parity(engine, max_lag, k):
    # max_lag + k + 2: legal at max_lag 1 (its smallest shape), NOT_ENOUGH_DATA at 4; 2 max_lag + k + 1: the smallest
    for Tn in (max_lag + k + 2, 2 * max_lag + k + 1, T):
        rng = np.random.default_rng(100 * max_lag + 10 * k + Tn)
        u, f = rng.standard_normal((65, Tn)), rng.standard_normal((65, Tn, k))
        ref = [R.bgtest(u[i], f[i].T, max_lag) for i in range(65)]
        st = _check_test(engine.bgtest(u, f, max_lag), ref, ("bgtest", max_lag, k, Tn))
        assert np.all(st == (R.ST_OK if Tn >= 2 * max_lag + k + 1 else R.ST_NOT_ENOUGH_DATA))


@pytest.mark.parametrize("k", [1, 3])
def test_bptest_bit_parity(engine, k):
    for Tn in (k + 1, T):
        rng = np.random.default_rng(10 * k + Tn)
        u, f = rng.standard_normal((65, Tn)), rng.standard_normal((65, Tn, k))
        if Tn == T:
            f[9, :, 0] = 0.0                           # SINGULAR: NaN statistic and p-value
        ref = [R.bptest(u[i], f[i].T) for i in range(65)]
        st = _check_test(engine.bptest(u, f), ref, ("bptest", k, Tn))
        assert np.all(np.delete(st, 9) == R.ST_OK) and st[9] == (R.ST_SINGULAR if Tn == T else R.ST_OK)


def test_breusch_suites_on_the_device():
    from sparkts_amd import stats
    x, resids1, resids2 = bg_suite()
    f = np.array(x)[:, None]
    for lag in (1, 4):
        p = stats.bgtest(np.array([resids1, resids2]), f, lag)[1]
        assert p[0] > 0.05 and p[1] < 0.05, (lag, p)
    x, resids1, resids2 = bp_suite()
    stat, p = stats.bptest(np.array([resids1, resids2]), np.array(x)[:, None])
    assert p[0] > 0.05 and p[1] < 0.05, p
    ref = [R.bptest(r, [x]) for r in (resids1, resids2)]
    assert _same(stat, [r[1] for r in ref]) and _p_close(p, [r[2] for r in ref])


@pytest.mark.parametrize("name", ARX_SUITE_CASES)
def test_arx_suite_on_the_device(arx_suite, name):  # noqa: F811
    from sparkts_amd.models import AutoregressionX
    X, _, intercept = arx_suite
    y, yl, xl, orig, want = _suite_case(name, X, intercept)
    model = AutoregressionX.fit_model(y, np.array(X), yl, xl, include_original_x=orig)
    assert abs(model.c - intercept) <= SUITE_TOL
    assert model.coefficients.shape == (len(want),) and np.all(np.abs(model.coefficients - want) <= SUITE_TOL)


def test_arx_suite_predict_on_the_device():
    from sparkts_amd.models import AutoregressionX
    model = AutoregressionX.ARXModel(0, PREDICT_COEFFS, 0, 0, includes_original_x=True)
    out = model.predict([100.0], np.array([PREDICT_X]))
    assert out.shape == (1,) and abs(out[0] - 100.0) <= SUITE_TOL
    assert _same(out, R.arx_predict([100.0], [[v] for v in PREDICT_X], 0, PREDICT_COEFFS, 0, 0, True))
    with pytest.raises(AutoregressionX.ARIMAFitError):
        AutoregressionX.fit_model([1.0, 2.0, 3.0], np.zeros((3, 1)), 0, 0)      # a zero column: SingularMatrixException


# ---- 4. slices ------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_slice_size(engine):
    cfg = CONFIGS[5]
    yl, xl, k, orig, noint = cfg
    y, x = _arx_case(cfg)[:2]
    x = x.copy()
    x[129, :, 2] = 0.0                                 # a failure in the last, partial slice
    calls = (lambda: engine.arx_fit(y, x, yl, xl, orig, noint), lambda: engine.bgtest(y, x, 2),
             lambda: engine.bptest(y, x))
    whole = [c() for c in calls]
    before = engine.get_option("regress_slice_bytes")
    assert before == 0
    engine.set_option("regress_slice_bytes", 1)        # one block of 64 series per slice: 64 + 64 + 2
    try:
        sliced = [c() for c in calls]
    finally:
        engine.set_option("regress_slice_bytes", before)
    for a, b in zip(whole, sliced):
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(a[key], b[key]) if key == "status" else _same(a[key], b[key]), key
    assert whole[0]["status"][129] == R.ST_SINGULAR


# ---- 5. the device entry points ---------------------------------------------------------------------------------
def _padded(a, ld, torch):
    host = np.full((a.shape[0], ld), np.nan)           # padding columns must never be consumed
    host[:, :a.shape[1]] = a
    return torch.from_numpy(host).cuda()


def test_device_variants_equal_the_host_variants(engine):
    import torch
    cfg = CONFIGS[5]
    yl, xl, k, orig, noint = cfg
    N, ld = 70, T + 3
    y, x = (a[:N] for a in _arx_case(cfg)[:2])
    K = engine.arx_num_coef(k, yl, xl, orig)
    Rr = T - max(yl, xl)
    host = engine.arx_fit(y, x, yl, xl, orig, noint)
    host_pred = engine.arx_predict(y, x, yl, xl, orig, host["coef"])
    host_bg, host_bp = engine.bgtest(y, x, 2), engine.bptest(y, x)
    sd = _padded(y, ld, torch)
    xs = k * T + 5                                     # a series stride above n_xcols * T
    xh = np.full((N, xs), np.nan)
    xh[:, :k * T] = x.transpose(0, 2, 1).reshape(N, k * T)
    xd = torch.from_numpy(xh).cuda()
    coef = torch.full((N * (1 + K) + 8,), SENT, dtype=torch.float64, device="cuda")
    status = torch.full((N + 8,), -7, dtype=torch.int32, device="cuda")
    pred = torch.full((N, Rr + 3), SENT, dtype=torch.float64, device="cuda")
    vec = [torch.full((N + 8,), SENT, dtype=torch.float64, device="cuda") for _ in range(4)]
    sts = [torch.full((N + 8,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = stream.cuda_stream
    engine.arx_fit_device(sd.data_ptr(), N, T, ld, xd.data_ptr(), xs, k, yl, xl, orig, noint, coef.data_ptr(),
                          status.data_ptr(), stream=s, blocking=False)
    engine.arx_predict_device(sd.data_ptr(), N, T, ld, xd.data_ptr(), xs, k, yl, xl, orig, coef.data_ptr(),
                              pred.data_ptr(), Rr + 3, stream=s, blocking=False)
    engine.bgtest_device(sd.data_ptr(), N, T, ld, xd.data_ptr(), xs, k, 2, vec[0].data_ptr(), vec[1].data_ptr(),
                         sts[0].data_ptr(), stream=s, blocking=False)
    engine.bptest_device(sd.data_ptr(), N, T, ld, xd.data_ptr(), xs, k, vec[2].data_ptr(), vec[3].data_ptr(),
                         sts[1].data_ptr(), stream=s)
    c, st, pr = coef.cpu().numpy(), status.cpu().numpy(), pred.cpu().numpy()
    assert np.all(c[N * (1 + K):] == SENT) and np.all(st[N:] == -7), "written past an output"
    assert np.all(pr[:, Rr:] == SENT), "written past a prediction row"
    assert _same(c[:N * (1 + K)].reshape(N, 1 + K), host["coef"]) and np.array_equal(st[:N], host["status"])
    assert _same(pr[:, :Rr], host_pred)
    v = [a.cpu().numpy() for a in vec]
    assert all(np.all(a[N:] == SENT) for a in v)
    for got_s, got_p, got_st, want in ((v[0], v[1], sts[0], host_bg), (v[2], v[3], sts[1], host_bp)):
        assert _same(got_s[:N], want["stat"]) and _same(got_p[:N], want["pvalue"])
        assert np.array_equal(got_st.cpu().numpy()[:N], want["status"])


def test_device_variants_refuse_overlapping_buffers(engine):
    import torch
    N, k = 8, 2
    sd = torch.zeros((N, T), dtype=torch.float64, device="cuda")
    xd = torch.zeros((k, T), dtype=torch.float64, device="cuda")
    out = torch.zeros((N * 8,), dtype=torch.float64, device="cuda")
    st = torch.zeros((N,), dtype=torch.int32, device="cuda")
    Lb, h = engine.L, engine.h
    def fit(coef, status):
        return Lb.arima_arx_fit_batch_device(h, sd.data_ptr(), N, T, T, xd.data_ptr(), 0, k, 1, 0, 1, 0, coef, status,
                                             None)

    assert fit(out.data_ptr(), st.data_ptr()) == L.ARIMA_OK
    assert fit(sd.data_ptr(), st.data_ptr()) == L.ARIMA_E_INVALID_ARG              # coef_out over the series
    assert fit(xd.data_ptr(), st.data_ptr()) == L.ARIMA_E_INVALID_ARG              # ... over the regressors
    assert fit(out.data_ptr(), out.data_ptr() + 8) == L.ARIMA_E_INVALID_ARG        # status_out inside coef_out
    assert Lb.arima_arx_predict_batch_device(h, sd.data_ptr(), N, T, T, xd.data_ptr(), 0, k, 1, 0, 1, out.data_ptr(),
                                             out.data_ptr() + 16, T - 1, None) == L.ARIMA_E_INVALID_ARG
    def test(stat, p, status):
        return Lb.arima_bgtest_batch_device(h, sd.data_ptr(), N, T, T, xd.data_ptr(), 0, k, 1, stat, p, status, None)

    assert test(out.data_ptr(), out.data_ptr() + 8 * N, st.data_ptr()) == L.ARIMA_OK
    assert test(out.data_ptr(), out.data_ptr() + 8, st.data_ptr()) == L.ARIMA_E_INVALID_ARG   # the two outputs meet
    assert test(sd.data_ptr(), out.data_ptr(), st.data_ptr()) == L.ARIMA_E_INVALID_ARG
    assert Lb.arima_bptest_batch_device(h, sd.data_ptr(), N, T, T, xd.data_ptr(), 0, k, out.data_ptr(), xd.data_ptr(),
                                        st.data_ptr(), None) == L.ARIMA_E_INVALID_ARG
    engine.synchronize()


def test_bad_arguments(engine):
    y, x = np.zeros((4, T)), np.zeros((T, 2))
    xt = np.ascontiguousarray(x.T)
    coef, st = np.empty((4, 80)), np.empty(4, dtype=np.int32)
    for k, yl, xl in ((2, -1, 0), (2, 0, -1), (-1, 0, 0)):
        assert engine.L.arima_arx_fit_batch(engine.h, L._ptr(y), 4, T, L._ptr(xt), 0, k, yl, xl, 1, 0, L._ptr(coef),
                                            L._ptr(st, L._i32p)) == L.ARIMA_E_INVALID_ARG, (k, yl, xl)
    assert engine.L.arima_arx_fit_batch(engine.h, L._ptr(y), 4, T, L._ptr(xt), T, 2, 0, 0, 1, 0, L._ptr(coef),
                                        L._ptr(st, L._i32p)) == L.ARIMA_E_INVALID_ARG      # stride below n_xcols * T
    with pytest.raises(L.EngineError):
        engine.arx_fit(y, x, -1, 0)
    with pytest.raises(L.EngineError, match=r"\(-1\)"):
        engine.bgtest(y, x, 0)
    with pytest.raises(L.EngineError, match=r"\(-1\)"):
        engine.bptest(y, np.zeros((T, 0)))
    with pytest.raises(L.EngineError, match=r"\(-1\)"):
        engine.arx_predict(y, x, T + 1, 0, True, np.zeros(1 + T + 1 + 2))      # T < maxLag
    with pytest.raises(L.EngineError, match=r"\(-2\)"):
        engine.arx_fit(y, x, 62, 0)                    # 1 + 62 + 2 = 65 columns
    assert np.all(engine.arx_fit(y, x, 61, 0)["status"] == R.ST_SERIES_TOO_SHORT)     # 64 columns: a legal call
    assert engine.L.arima_arx_num_coef(-1, 0, 0, 1) == L.ARIMA_E_INVALID_ARG
    assert engine.arx_num_coef(3, 3, 2, True) == 12
    # N == 0 writes nothing
    assert engine.arx_fit(np.zeros((0, T)), x, 1, 0)["coef"].shape == (0, 4)
