"""Batched ARIMAX fits and forecasts on the device (csrc/arima_arimax.hip) against the CPU restatement
tests/arimax_ref.py, bit for bit: coefficient bit patterns with NaNs in the same places, ll, status, n_eval, n_grad and
the forecasts. The inputs and their restated results come from tests/arimax_cases.py, computed once per process;
tests/test_arimax_ref.py checks the conditions they have to meet."""
import numpy as np
import pytest

import arimax_cases as C
import arimax_ref as AX
import regress_ref as R
import sparkts_amd._lib as L
from test_gpu_diag import _same

pytestmark = pytest.mark.gpu

FIT_KEYS = ("coef", "ll", "status", "n_eval", "n_grad")


def _check_fit(got, ref, what, n=None):
    for key in ("status", "n_eval", "n_grad"):
        assert np.array_equal(got[key], ref[key][:n]), (what, key, got[key], ref[key][:n])
    assert _same(got["ll"], ref["ll"][:n]), (what, "ll")
    assert _same(got["coef"], ref["coef"][:n]), (what, "coef")
    failed = ref["status"][:n] != AX.ST_OK
    assert np.all(np.isnan(got["coef"][failed])) and np.all(np.isnan(got["ll"][failed])), what


def _same_fit(a, b):
    return all(_same(a[k], b[k]) if a[k].dtype == np.float64 else np.array_equal(a[k], b[k]) for k in FIT_KEYS)


@pytest.fixture
def smear_option(engine):
    before = engine.get_option("smear")
    yield lambda v: engine.set_option("smear", v)
    engine.set_option("smear", before)


# ---- 1. parity of the fits ----------------------------------------------------------------------------------------
def _fit_params():
    return [(cfg, smear) for cfg in sorted(C.CONFIGS) for smear in ((1, 0) if C.CONFIGS[cfg][2] == 2 else (1,))]


@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("cfg,smear", _fit_params(), ids=lambda v: str(v))
def test_fit_bit_parity(engine, smear_option, cfg, smear, N):
    p, d, q, Lx, orig, icpt, T, k = C.CONFIGS[cfg]
    y, x = C.batch(cfg)
    smear_option(smear)
    got = engine.arimax_fit(y[:N], x[:N], p, d, q, Lx, orig, icpt)
    assert got["coef"].shape == (N, AX.num_coef(k, p, q, Lx, orig))
    _check_fit(got, C.batch_ref(cfg, smear), (cfg, smear, N), N)


def test_user_init_skips_the_start_point(engine):
    p, d, q, Lx, orig, icpt, T, k = C.CONFIGS["a"]
    y, x, init, ref = C.user_init_case()
    got = engine.arimax_fit(y, x, p, d, q, Lx, orig, icpt, user_init=init)
    _check_fit(got, ref, "user_init")
    # one start for every series, and a start where the regression would have refused the series
    one = engine.arimax_fit(y[:3], x[:3], p, d, q, Lx, orig, icpt, user_init=init[1])
    _check_fit(one, AX.arimax_fit_batch(y[:3], C.x_columns(x[:3]), p, d, q, Lx, orig, icpt, user_init=init[1]), "one")
    ones = x[:2].copy()
    ones[:, :, 0] = 1.0
    assert np.all(engine.arimax_fit(y[:2], ones, p, d, q, Lx, orig, icpt)["status"] == R.ST_SINGULAR)
    assert _same_fit(engine.arimax_fit(y[:2], ones, p, d, q, Lx, orig, icpt, user_init=init[:2]),
                     {key: v[:2] for key, v in got.items()})


def test_shared_matrix_equals_its_copies(engine):
    p, d, q, Lx, orig, icpt, T, k = C.CONFIGS["a"]
    y, x = C.batch("a", True)
    assert x.shape == (T, k)
    a = engine.arimax_fit(y, x, p, d, q, Lx, orig, icpt)
    b = engine.arimax_fit(y, np.ascontiguousarray(np.broadcast_to(x, (len(y), T, k))), p, d, q, Lx, orig, icpt)
    assert _same_fit(a, b)
    _check_fit(a, C.batch_ref("a", 1, True), "shared")


@pytest.mark.parametrize("cfg,shared", [("a", False), ("a", True), ("b", False)])
def test_results_do_not_depend_on_the_slice_size(engine, cfg, shared):
    p, d, q, Lx, orig, icpt, T, k = C.CONFIGS[cfg]
    y, x = C.batch(cfg, shared)
    whole = engine.arimax_fit(y, x, p, d, q, Lx, orig, icpt)
    before = engine.get_option("regress_slice_bytes")
    engine.set_option("regress_slice_bytes", 1)        # one block of 64 series per slice: 64 + 64 + 2
    try:
        sliced = engine.arimax_fit(y, x, p, d, q, Lx, orig, icpt)
    finally:
        engine.set_option("regress_slice_bytes", before)
    assert _same_fit(whole, sliced)
    _check_fit(whole, C.batch_ref(cfg, 1, shared), (cfg, shared))


# ---- 2. failing lanes next to healthy ones ------------------------------------------------------------------------
def test_failing_lanes_next_to_healthy_ones(engine):
    p, d, q, Lx, orig, icpt, T, k = C.CONFIGS["a"]
    y, x, ref = C.edge_batch()
    got = engine.arimax_fit(y, x, p, d, q, Lx, orig, icpt)
    _check_fit(got, ref, "edges")
    for name in ("ones-column", "ones-column-2"):
        i = C.EDGE_LANES[name]
        assert got["status"][i] == R.ST_SINGULAR and got["n_eval"][i] == 0 and got["n_grad"][i] == 0
    keep = np.delete(np.arange(len(y)), list(C.EDGE_LANES.values()))
    alone = engine.arimax_fit(y[keep], x[keep], p, d, q, Lx, orig, icpt)
    assert _same_fit(alone, {key: v[keep] for key, v in got.items()})


@pytest.mark.parametrize("name", sorted(C.SHORT_CASES))
def test_series_too_short(engine, name):
    (p, d, q, Lx, orig, icpt, T, k), arx_st, hr_st = C.SHORT_CASES[name]
    y, x, ref = C.short_case(name)
    got = engine.arimax_fit(y, x, p, d, q, Lx, orig, icpt)
    _check_fit(got, ref, name)
    assert np.all(got["status"] == (arx_st or hr_st)) and np.all(got["n_eval"] == 0)


def test_widest_fit_and_one_beyond(engine):
    p, d, q, Lx, orig, icpt, T, k = C.WIDE
    y, x, ref = C.wide_case()
    got = engine.arimax_fit(y, x, p, d, q, Lx, orig, icpt)
    assert got["coef"].shape == (3, 41)
    _check_fit(got, ref, "K' = 41")
    with pytest.raises(L.EngineError, match=r"\(-2\)"):
        engine.arimax_fit(y, x, p + 1, d, q, Lx, orig, icpt)               # K' = 42
    with pytest.raises(L.EngineError, match=r"\(-2\)"):
        engine.arimax_fit(y, x[:, :, :1], 21, d, q, 0, orig, icpt)          # p above the runtime-order limit


# ---- 3. forecasts -------------------------------------------------------------------------------------------------
def _shape_id(s):
    return "T%d-nF%s-d%d-%s-L%d-%s-p%dq%d-k%d" % (s[0], s[1], s[2], "orig" if s[3][0] else "lags", s[3][1],
                                                   "c" if s[3][2] else "noc", s[4][0], s[4][1], s[5])


# the streaming kernel (forecast_shapes: p, q <= 5, d <= 8) and the workspace kernel above those orders
@pytest.mark.parametrize("shape", C.forecast_shapes() + C.FC_WORKSPACE_SHAPES, ids=_shape_id)
def test_forecast_bit_parity(engine, shape):
    T, rule, d, (orig, Lx, icpt), (p, q), k = shape
    y, x, coef, ref = C.forecast_case(shape)
    got = engine.arimax_forecast(y, x, p, d, q, Lx, orig, icpt, coef)
    assert got.shape == (C.FC_N, T) and _same(got, ref)
    for N in (1, 64):
        assert _same(engine.arimax_forecast(y[:N], x[:N], p, d, q, Lx, orig, icpt, coef[:N]), ref[:N]), N
    # one matrix and one model for every series
    shared = engine.arimax_forecast(y[:3], x[1], p, d, q, Lx, orig, icpt, coef[2])
    assert _same(shared, AX.arimax_forecast_batch(y[:3], C.x_columns(x[1]), p, d, q, Lx, orig, icpt, coef[2]))


def test_forecast_workspace_slices(engine):
    """More series than one slice of the forecast workspace: the second launch starts inside the batch, at series sl,
    with the series, the regressors, the coefficients and the output each offset by their own stride."""
    import torch
    T, nF, d, (orig, Lx, icpt), (p, q), k = C.SLICE_SHAPE
    y, x, coef, sl, ref = C.slice_case()
    N, W, R4 = C.SLICE_N, C.SLICE_WINDOW, C.SLICE_REF
    assert sl < N < 2 * sl                                   # a second launch, or the test tests nothing
    win = slice(sl - W, sl + W)
    whole = engine.arimax_forecast(y, x, p, d, q, Lx, orig, icpt, coef)
    assert whole.shape == (N, T)
    alone = engine.arimax_forecast(y[win], x[win], p, d, q, Lx, orig, icpt, coef[win])
    assert _same(whole[win], alone)
    assert _same(whole[sl - R4:sl + R4], ref)
    # the device entry: strided rows and matrices (NaN padding behind each), a strided output with guard columns
    ld, xs, ld_out = T + 3, k * nF + 3, T + 5
    buf = torch.full((N, ld), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :T] = torch.tensor(y, device="cuda")
    dx = torch.full((N, xs), float("nan"), dtype=torch.float64, device="cuda")
    dx[:, :k * nF] = torch.tensor(np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(N, k * nF), device="cuda")
    dcoef = torch.tensor(coef, device="cuda")
    dout = torch.full((N, ld_out), -7.0, dtype=torch.float64, device="cuda")
    engine.arimax_forecast_device(buf.data_ptr(), N, T, ld, dx.data_ptr(), xs, k, nF, p, d, q, Lx, orig, icpt,
                                  dcoef.data_ptr(), dout.data_ptr(), ld_out)
    got = dout.cpu().numpy()
    assert np.all(got[:, T:] == -7.0), np.argwhere(got[:, T:] != -7.0)[:4]
    assert _same(got[win, :T], alone) and _same(got[sl - R4:sl + R4, :T], ref)
    assert _same(got[:, :T], whole)
    assert torch.isnan(buf[:, T:]).all() and torch.isnan(dx[:, k * nF:]).all()


def test_forecast_invalid_shapes(engine):
    y, coef = np.ones((2, 40)), np.full((2, 41), 0.1)

    def call(T=40, k=2, nF=5, p=1, d=0, q=1, Lx=1):
        x = np.ones((2, max(k, 1) * max(nF, 1)))
        out = np.empty((2, 40))
        return engine.L.arima_arimax_forecast_batch(engine.h, L._ptr(y), 2, T, L._ptr(x), 0, k, nF, p, d, q, Lx, 1, 1,
                                                    L._ptr(coef), L._ptr(out))

    assert call() == L.ARIMA_OK
    assert call(p=0, q=0) == L.ARIMA_E_INVALID_ARG                          # xregPredictors(-1)
    assert call(k=0) == L.ARIMA_E_INVALID_ARG and call(k=-1) == L.ARIMA_E_INVALID_ARG
    assert call(T=20, nF=24, Lx=3) == L.ARIMA_E_INVALID_ARG                 # nFuture - L > T
    assert call(T=20, nF=23, Lx=3) == L.ARIMA_OK
    assert call(nF=0, Lx=2) == L.ARIMA_E_INVALID_ARG                        # R - L < 0
    assert call(nF=0, Lx=1) == L.ARIMA_OK
    assert call(T=1, d=2) == L.ARIMA_E_INVALID_ARG
    for kw in (dict(p=-1), dict(d=-1), dict(q=-1), dict(Lx=-1), dict(nF=-1), dict(T=-1)):
        assert call(**kw) == L.ARIMA_E_INVALID_ARG, kw
    assert call(p=21) == L.ARIMA_E_UNSUPPORTED and call(d=17, T=40) == L.ARIMA_E_UNSUPPORTED
    assert call(k=6, Lx=6) == L.ARIMA_E_UNSUPPORTED                          # K' = 45
    with pytest.raises(L.EngineError, match=r"\(-1\)"):
        engine.arimax_forecast(y, np.ones((5, 2)), 0, 0, 0, 1, True, True, coef[:, :5])
    # the model raises what the restatement raises
    from sparkts_amd.models import ARIMAX
    for kw in (dict(p=0, q=0), dict(d=41), dict(Lx=7), dict(Lx=0, nF=42)):
        a = dict(p=1, d=0, q=1, Lx=1, nF=5)
        a.update(kw)
        m = ARIMAX.ARIMAXModel(a["p"], a["d"], a["q"], a["Lx"], np.full(AX.num_coef(2, a["p"], a["q"], a["Lx"]), 0.1))
        with pytest.raises(ValueError):
            AX.arimax_forecast(y[0], [[1.0] * a["nF"]] * 2, a["p"], a["d"], a["q"], a["Lx"], True, True, m.coefficients)
        with pytest.raises(ValueError):
            m.forecast(y[0], np.ones((a["nF"], 2)))


# ---- 4. the Python layer ------------------------------------------------------------------------------------------
def test_python_layer_on_the_first_suite_case(engine):
    from sparkts_amd.models import ARIMA, ARIMAX
    from sparkts_amd.models.ARIMA import SingularMatrixException
    c = C.suite_cases()[0]
    ts, x, ts_test, x_test = C.suite_data()[c["data"]]
    ref = C.suite_fit(0, engine.get_option("smear"))
    model = ARIMAX.fit_model(c["p"], c["d"], c["q"], ts, np.array(x).T, c["xreg_max_lag"])
    assert model.coefficients.shape == (c["num_coef"],) and _same(model.coefficients, ref["coef"])
    f = model.forecast(ts_test, np.array(x_test).T)
    want = AX.arimax_forecast(ts_test, x_test, c["p"], c["d"], c["q"], c["xreg_max_lag"], True, True, ref["coef"])
    assert f.shape == (len(ts_test),) and _same(f, want)
    avg = sum(ts_test) / len(ts_test)
    assert np.all(np.abs(f - avg) <= c["tolerance"])                        # what the reference suite asserts
    assert _same(model.forecast_batch(np.array([ts_test, ts_test]), np.array(x_test).T), [want, want])
    # the effects pair and the log-likelihood are ARIMA's on the coefficient prefix
    ka = 1 + c["p"] + c["q"]
    plain = ARIMA.ARIMAModel(c["p"], c["d"], c["q"], model.coefficients[:ka], True)
    noise = np.random.default_rng(1).standard_normal(30)
    assert _same(model.add_time_dependent_effects(noise), plain.add_time_dependent_effects(noise))
    assert _same(model.remove_time_dependent_effects(np.array(ts)), plain.remove_time_dependent_effects(np.array(ts)))
    assert model.log_likelihood_css_arma(np.array(ts)) == plain.log_likelihood_css_arma(np.array(ts)) == ref["ll"]
    # a model without an intercept reads its effects from slot 0 on
    noc = ARIMAX.ARIMAXModel(1, 0, 1, 1, [0.3, 0.2, 9.0, 9.0, 9.0, 9.0], True, False)
    assert _same(noc.add_time_dependent_effects(noise),
                 ARIMA.ARIMAModel(1, 0, 1, [0.3, 0.2], False).add_time_dependent_effects(noise))
    # failures: the reference's exception for one series, a status per series for a batch
    ones = np.array(x).T.copy()
    ones[:, 0] = 1.0
    with pytest.raises(SingularMatrixException) as e:
        ARIMAX.fit_model(0, 0, 1, ts, ones, 1)
    assert e.value.status == R.ST_SINGULAR
    r = ARIMAX.fit_models(0, 0, 1, np.array([ts, ts]), np.stack([np.array(x).T, ones]), 1)
    assert r.converged.tolist() == [True, False] and _same(r.model(0).coefficients, ref["coef"])
    with pytest.raises(SingularMatrixException):
        r.model(1)
    init = np.asarray(ref["init"]) * 1.01
    u = ARIMAX.fit_model(0, 0, 1, ts, np.array(x).T, 1, user_init_params=init)
    assert _same(u.coefficients, AX.arimax_fit(ts, x, 0, 0, 1, 1, user_init=init,
                                               smear=engine.get_option("smear"))["coef"])
