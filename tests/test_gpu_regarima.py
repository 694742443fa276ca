"""Batched RegressionARIMA (Cochrane-Orcutt) fits on the device (k_cochrane_orcutt, csrc/arima_regress.hip) against
the CPU restatement tests/regarima_ref.py: coefficients and rho bit for bit (NaNs in the same places), the statuses
and iteration counts equal. Lanes of one wave leave the loop at different iterations, for different reasons or with a
failure: the batches hold all of these side by side."""
import numpy as np
import pytest

import regarima_ref as C
import regress_ref as R
import sparkts_amd._lib as L
from test_gpu_diag import _same
from test_regarima_ref import (EDGE_K, EDGE_T, PARITY_SHAPES, SUITE_CASES, ar1_batch, check_suite, edge_batch,
                               parity_case, shape_edge, suite_case)

pytestmark = pytest.mark.gpu

SENT = -7.0


def _check(got, ref, what, n=None):
    coef, rho, n_iter, status = (np.array(a[:n]) for a in ref[:4])
    assert np.array_equal(got["status"], status.astype(np.int32)), (what, got["status"], status)
    assert np.array_equal(got["n_iter"], n_iter.astype(np.int32)), (what, got["n_iter"], n_iter)
    assert _same(got["rho"], rho), what
    assert _same(got["coef"], coef.reshape(len(status), -1)), what
    failed = status != R.ST_OK
    assert np.all(np.isnan(got["coef"][failed])) and np.all(np.isnan(got["rho"][failed])), what


# ---- 1. parity: every stopping reason inside one wave ---------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("shape", PARITY_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_fit_bit_parity(engine, shape, N):
    T, k, max_iter = shape
    y, x, ref = parity_case(shape)
    # from the restatement alone: the batch holds the four ways out of the loop (a batch without one is a broken
    # fixture)
    reasons = {C.reason(f, max_iter) for f in ref[4]}
    assert reasons == {C.STOP_BEFORE_LOOP, C.STOP_DW, C.STOP_RHO, C.STOP_MAX_ITER}, reasons
    _check(engine.regarima_co_fit(y[:N], x[:N], max_iter), ref, (shape, N), N)


def test_rows_beyond_one_tile_and_the_widest_design(engine):
    # T = 70: the pristine copy comes through three 32-row tiles, the last one partial; per series and shared
    y, x = ar1_batch(np.random.default_rng(70), 65, 70, 2)
    ref = C.fit_batch(y, x, 4)
    assert len(set(ref[2])) >= 3
    _check(engine.regarima_co_fit(y, x, 4), ref, "T = 70")
    _check(engine.regarima_co_fit(y, x[0], 4), C.fit_batch(y, x[0], 4), "T = 70, shared")
    # C = 64 design columns, the 64 KiB launch: k = 63, one series that iterates and one whose NaN ends it at once
    y, x = ar1_batch(np.random.default_rng(64), 2, 66, 63, phis=(0.95,))
    y[1, 7] = np.nan
    ref = C.fit_batch(y, x, 2)
    assert ref[2] == [2, 0] and ref[3] == [R.ST_OK, R.ST_OK]
    _check(engine.regarima_co_fit(y, x, 2), ref, "C = 64")


# ---- 2. edges: a failed or NaN lane next to healthy ones ----------------------------------------------------------------
def test_edges_in_one_batch(engine):
    y, x, where = edge_batch()
    ref = C.fit_batch(y, x)
    got = engine.regarima_co_fit(y, x)
    _check(got, ref, "edges")
    assert got["status"][where["constant-column"]] == R.ST_SINGULAR
    i = where["exactly-linear"]
    assert (got["n_iter"][i], got["rho"][i]) == (0, 0.0) and got["coef"][i].tolist() == [2.0, 3.0, -4.0]
    for name in ("nan-in-y", "nan-in-x", "inf-in-y"):
        assert got["status"][where[name]] == R.ST_OK and np.all(np.isnan(got["coef"][where[name]])), name
    # the neighbours are what they are without the edge series
    keep = np.array([j for j in range(len(y)) if j not in where.values()])
    alone = engine.regarima_co_fit(y[keep], x[keep])
    for key in ("coef", "rho"):
        assert _same(alone[key], got[key][keep]) and not np.any(np.isnan(alone[key])), key
    assert np.array_equal(alone["n_iter"], got["n_iter"][keep]) and np.any(alone["n_iter"] > 0)


@pytest.mark.parametrize("T,k", [(3, 2), (4, 3), (2, 2), (3, 3), (0, 1), (0, 3)])
def test_shape_edges(engine, T, k):
    y, x = shape_edge(T, k)
    ref = C.fit_batch(y, x)
    _check(engine.regarima_co_fit(y, x), ref, (T, k))
    if T == k + 1:
        assert set(ref[3]) <= {R.ST_OK, R.ST_NOT_ENOUGH_DATA}
    else:
        assert set(ref[3]) == {R.ST_NO_DATA if T == 0 else R.ST_NOT_ENOUGH_DATA}


# ---- 3. max_iter ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [1, 2, 11])
def test_max_iter(engine, max_iter):
    y, x = (a[:70] for a in parity_case(PARITY_SHAPES[0])[:2])
    ref = C.fit_batch(y, x, max_iter)
    assert max(ref[2]) == max_iter
    _check(engine.regarima_co_fit(y, x, max_iter), ref, max_iter)


def test_bad_arguments(engine):
    T = 12
    y, x = np.zeros((4, T)), np.zeros((2, T))
    coef, rho = np.empty((4, 80)), np.empty(4)
    it, st = np.empty(4, dtype=np.int32), np.empty(4, dtype=np.int32)

    def call(k, max_iter, xs=0):
        return engine.L.arima_regarima_co_fit_batch(engine.h, L._ptr(y), 4, T, L._ptr(x), xs, k, max_iter, L._ptr(coef),
                                                    L._ptr(rho), L._ptr(it, L._i32p), L._ptr(st, L._i32p))

    assert call(2, 1) == L.ARIMA_OK
    for max_iter in (0, -1):
        assert call(2, max_iter) == L.ARIMA_E_INVALID_ARG
    assert call(0, 10) == L.ARIMA_E_INVALID_ARG and call(-1, 10) == L.ARIMA_E_INVALID_ARG
    assert call(2, 10, xs=2 * T - 1) == L.ARIMA_E_INVALID_ARG               # a stride in (0, k T)
    with pytest.raises(L.EngineError, match=r"\(-1\)"):
        engine.regarima_co_fit(y, x.T, 0)
    with pytest.raises(L.EngineError, match=r"\(-2\)"):
        engine.regarima_co_fit(y, np.zeros((T, 64)))                        # 65 design columns
    assert np.all(engine.regarima_co_fit(y, np.zeros((T, 63)))["status"] == R.ST_NOT_ENOUGH_DATA)   # 64: a legal call
    assert engine.regarima_co_fit(np.zeros((0, T)), x.T)["coef"].shape == (0, 3)                 # N == 0


# ---- 4. shared x, slices ------------------------------------------------------------------------------------------------
def test_shared_x_equals_copies(engine):
    T, k, max_iter = PARITY_SHAPES[0]
    y = parity_case(PARITY_SHAPES[0])[0]
    x = np.random.default_rng(5).standard_normal((T, k))
    per = np.ascontiguousarray(np.broadcast_to(x, (len(y), T, k)))
    a, b = engine.regarima_co_fit(y, x, max_iter), engine.regarima_co_fit(y, per, max_iter)
    for key in a:
        assert _same(a[key], b[key]) if a[key].dtype == np.float64 else np.array_equal(a[key], b[key]), key
    _check({key: v[:5] for key, v in a.items()}, C.fit_batch(y[:5], x, max_iter), "shared x")


def test_results_do_not_depend_on_the_slice_size(engine):
    T, k, max_iter = PARITY_SHAPES[0]
    y, x = parity_case(PARITY_SHAPES[0])[:2]
    x = x.copy()
    x[129, :, 1] = 0.0                                 # a failure in the last, partial slice
    whole = engine.regarima_co_fit(y, x, max_iter)
    before = engine.get_option("regress_slice_bytes")
    assert before == 0
    engine.set_option("regress_slice_bytes", 1)        # one block of 64 series per slice: 64 + 64 + 2
    try:
        sliced = engine.regarima_co_fit(y, x, max_iter)
    finally:
        engine.set_option("regress_slice_bytes", before)
    for key in whole:
        assert _same(whole[key], sliced[key]) if whole[key].dtype == np.float64 else \
            np.array_equal(whole[key], sliced[key]), key
    assert whole["status"][129] == R.ST_SINGULAR and np.all(whole["status"][:129] == R.ST_OK)


# ---- 5. the device entry point ------------------------------------------------------------------------------------------
def test_device_variant_on_a_caller_stream(engine):
    import torch
    T, k, max_iter = PARITY_SHAPES[0]
    N, ld = 70, T + 3
    y, x = (a[:N] for a in parity_case(PARITY_SHAPES[0])[:2])
    host = engine.regarima_co_fit(y, x, max_iter)
    yh = np.full((N, ld), SENT)
    yh[:, :T] = y
    yd = torch.from_numpy(yh).cuda()
    xs = k * T + 5                                     # a series stride above n_xcols * T
    xh = np.full((N, xs), SENT)
    xh[:, :k * T] = x.transpose(0, 2, 1).reshape(N, k * T)
    xd = torch.from_numpy(xh).cuda()
    coef = torch.full((N * (1 + k) + 8,), SENT, dtype=torch.float64, device="cuda")
    rho = [torch.full((N + 8,), SENT, dtype=torch.float64, device="cuda") for _ in range(2)]
    ints = [torch.full((N + 8,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = stream.cuda_stream
    engine.regarima_co_fit_device(yd.data_ptr(), N, T, ld, xd.data_ptr(), xs, k, max_iter, coef.data_ptr(),
                                  rho[0].data_ptr(), ints[0].data_ptr(), ints[1].data_ptr(), stream=s, blocking=False)
    engine.regarima_co_fit_device(yd.data_ptr(), N, T, ld, xd.data_ptr(), xs, k, max_iter, coef.data_ptr(),
                                  rho[1].data_ptr(), None, ints[2].data_ptr(), stream=s)      # n_iter_out = NULL
    assert np.all(yd.cpu().numpy()[:, T:] == SENT) and np.all(xd.cpu().numpy()[:, k * T:] == SENT)
    assert np.array_equal(yd.cpu().numpy()[:, :T], y)
    c, r0, r1 = coef.cpu().numpy(), rho[0].cpu().numpy(), rho[1].cpu().numpy()
    it, st0, st1 = (a.cpu().numpy() for a in ints)
    assert np.all(c[N * (1 + k):] == SENT) and np.all(r0[N:] == SENT) and np.all(r1[N:] == SENT)
    assert np.all(it[N:] == -7) and np.all(st0[N:] == -7) and np.all(st1[N:] == -7), "written past an output"
    assert _same(c[:N * (1 + k)].reshape(N, 1 + k), host["coef"])
    assert _same(r0[:N], host["rho"]) and _same(r1[:N], host["rho"])
    assert np.array_equal(it[:N], host["n_iter"])
    assert np.array_equal(st0[:N], host["status"]) and np.array_equal(st1[:N], host["status"])


def test_device_variant_refuses_overlapping_buffers(engine):
    import torch
    N, k, T = 8, 2, 12
    sd = torch.zeros((N, T), dtype=torch.float64, device="cuda")
    xd = torch.zeros((k, T), dtype=torch.float64, device="cuda")
    out = torch.zeros((N * 8,), dtype=torch.float64, device="cuda")
    ints = torch.zeros((2 * N,), dtype=torch.int32, device="cuda")

    def fit(coef, rho, n_iter, status, ld=T):
        return engine.L.arima_regarima_co_fit_batch_device(engine.h, sd.data_ptr(), N, T, ld, xd.data_ptr(), 0, k, 10,
                                                           coef, rho, n_iter, status, None)

    o, i = out.data_ptr(), ints.data_ptr()
    assert fit(o, o + 8 * 3 * N, i, i + 4 * N) == L.ARIMA_OK
    assert fit(sd.data_ptr(), o, i, i + 4 * N) == L.ARIMA_E_INVALID_ARG     # coef_out over the series
    assert fit(o, xd.data_ptr(), i, i + 4 * N) == L.ARIMA_E_INVALID_ARG     # rho_out over the regressors
    assert fit(o, o + 8, i, i + 4 * N) == L.ARIMA_E_INVALID_ARG             # rho_out inside coef_out
    assert fit(o, o + 8 * 3 * N, i, i + 4) == L.ARIMA_E_INVALID_ARG         # status_out inside n_iter_out
    assert fit(o, o + 8 * 3 * N, i, i + 4 * N, ld=T - 1) == L.ARIMA_E_INVALID_ARG
    engine.synchronize()


# ---- 6. the Python layer ------------------------------------------------------------------------------------------------
def test_python_layer(engine):
    from sparkts_amd.models import RegressionARIMA
    from sparkts_amd.models.ARIMA import SingularMatrixException, UnsupportedOperationException
    case = suite_case(SUITE_CASES[1])
    model = RegressionARIMA.fit_model(case["series"], np.array(case["regressor"]), "cochrane-orcutt", case["max_iter"])
    assert model.arima_orders.tolist() == [1, 0, 0] and model.arima_coeff.shape == (1,)
    check_suite(case, model.regression_coeff, model.arima_coeff[0], case["expected"]["n_iter"])
    st, beta, rho, n_iter, _ = C.cochrane_orcutt(case["series"], [case["regressor"]], case["max_iter"])
    assert _same(model.regression_coeff, beta) and _same(model.arima_coeff, [rho])
    case = suite_case(SUITE_CASES[0])
    one = RegressionARIMA.fit_model(case["series"], np.array(case["regressor"])[:, None], "cochrane-orcutt", 1)
    check_suite(case, one.regression_coeff, one.arima_coeff[0], 1)
    default = RegressionARIMA.fit_model(case["series"], case["regressor"], "cochrane-orcutt")
    assert _same(default.regression_coeff, C.cochrane_orcutt(case["series"], [case["regressor"]], 10)[1])
    with pytest.raises(UnsupportedOperationException) as e:
        RegressionARIMA.fit_model(case["series"], case["regressor"], "yule-walker")
    assert e.value.status == L.ST_UNSUPPORTED_METHOD
    with pytest.raises(ValueError, match="must be integer"):
        RegressionARIMA.fit_model(case["series"], case["regressor"], "cochrane-orcutt", 2.5)
    with pytest.raises(ValueError, match="can't exceed 3"):
        RegressionARIMA.fit_model(case["series"], case["regressor"], "cochrane-orcutt", 2, 3)
    with pytest.raises(SingularMatrixException):
        RegressionARIMA.fit_cochrane_orcutt([1.0, 2.0, 4.0, 3.0], np.zeros((4, 1)))
    for fn in (model.add_time_dependent_effects, model.remove_time_dependent_effects):
        with pytest.raises(NotImplementedError):
            fn(np.zeros(4), np.zeros(4))
    # the batched call never raises per series
    y, x, where = edge_batch()
    r = RegressionARIMA.fit_models(y, x)
    assert r.regression_coeff.shape == (len(y), 1 + EDGE_K) and r.rho.shape == r.n_iter.shape == (len(y),)
    assert not r.converged[where["constant-column"]] and r.converged.sum() == len(y) - 1
    with pytest.raises(SingularMatrixException):
        r.model(where["constant-column"])
    m = r.model(0)
    assert _same(m.regression_coeff, r.regression_coeff[0]) and m.arima_coeff[0] == r.rho[0] and EDGE_T == y.shape[1]
