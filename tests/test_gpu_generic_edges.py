"""The runtime-order path (spark-timeseries_amd/csrc/arima_generic.hip: p or q above 5, forecasts with d above 8) at its
edges, against the CPU restatement: integers exact, doubles bit for bit (_same, check_fit).

tests/test_gpu_generic.py fits well-conditioned mid-size batches; here are the lengths around every threshold of the
shape checks, a batch larger than the fixed grid (lanes that loop over several series), a forecast batch larger than
one workspace slice, forecasts of rows shorter than the model's orders, the maximum orders (20), the dispatch boundary
(5 | 6), special values next to clean rows in one wave, and null optional outputs. The inputs, and the CPU conditions
that keep each comparison from passing vacuously, are in tests/test_generic_edges_inputs.py.
"""
import numpy as np
import pytest

import oracle as O
import sparkts_amd._lib as L
import test_generic_edges_inputs as X
from test_gpu_parity import _same, check_fit

pytestmark = pytest.mark.gpu


# ---- 1. every length from 0 to a few past the first that fits ------------------------------------------------------
@pytest.mark.parametrize("order", X.SWEEP_ORDERS, ids=X.order_id)
def test_length_sweep_matches_oracle(engine, order):
    p, d, q, I = order
    rows, exp = X.sweep_rows(order), X.sweep_expect(order)
    try:
        for fuse in ((1, 0) if d == 1 else (1,)):            # d = 1: differenced inside the passes, or a copy
            engine.set_option("fuse_diff", fuse)
            for T in X.sweep_lengths(order):
                res = engine.fit_batch(rows[:, :T], p, d, q, bool(I))
                check_fit(res, exp[T], f"ARIMA{order} T={T} fuse_diff={fuse}")
    finally:
        engine.set_option("fuse_diff", 1)


# ---- 2. more series than the fixed grid has lanes ------------------------------------------------------------------
@pytest.mark.parametrize("order", X.STRIDE_ORDERS, ids=X.order_id)
def test_grid_stride_batch_matches_oracle(engine, order):
    # kGenGridMax workgroups of 64 lanes: above 262 144 series a lane fits a second series and adds its counters up.
    # The host path cuts a call into chunks of host_chunk series (at most 262 144 by default, and halves the last
    # two), so the whole batch goes in one chunk here: otherwise no launch would see more series than lanes.
    p, d, q, I = order
    rows, exp = X.stride_rows(), X.stride_expect(order)
    N = len(rows)
    saved = {k: engine.get_option(k) for k in ("host_chunk", "host_tail")}
    try:
        engine.set_option("host_chunk", N)
        engine.set_option("host_tail", 0)
        res = engine.fit_batch(rows, p, d, q, bool(I))
        st = engine.stats()
    finally:
        for k, v in saved.items():
            engine.set_option(k, v)
    assert N > X.GEN_GRID_MAX * X.GEN_BLOCK
    check_fit(res, exp, f"ARIMA{order} N={N}")
    assert st["series_done"] == N
    assert st["n_eval"] == int(res["n_eval"].sum(dtype=np.int64))
    assert st["n_grad"] == int(res["n_grad"].sum(dtype=np.int64))


# ---- 3. more series than one slice of the forecast workspace -------------------------------------------------------
def test_forecast_slices_match_oracle(engine):
    import torch
    p, d, q, I = X.SLICE_ORDER
    T, nf, N = X.SLICE_T, X.SLICE_NF, X.SLICE_N
    s, coef = X.slice_inputs()
    exp = X.slice_expect()
    sl = X.forecast_slice(N, T, p, d, q, nf)
    assert sl < N                                            # a second launch, at series sl, or the test tests nothing
    out = engine.forecast(s, p, d, q, I, coef, nf)
    assert _same(out[:sl], exp[:sl]) and _same(out[sl:], exp[sl:])
    # the device entry: strided rows (NaN padding behind each), a strided output with guard columns
    ld, ld_out = T + 3, T + nf + 5
    buf = torch.full((N, ld), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :T] = torch.tensor(s, device="cuda")
    dcoef = torch.tensor(coef, device="cuda")
    dout = torch.full((N, ld_out), -7.0, dtype=torch.float64, device="cuda")
    engine.forecast_device(buf.data_ptr(), N, T, ld, p, d, q, I, dcoef.data_ptr(), nf, dout.data_ptr(), ld_out)
    got = dout.cpu().numpy()
    assert np.all(got[:, T + nf:] == -7.0), np.argwhere(got[:, T + nf:] != -7.0)[:4]
    assert _same(got[:sl, :T + nf], exp[:sl]) and _same(got[sl:, :T + nf], exp[sl:])
    assert torch.isnan(buf[:, T:]).all() and np.array_equal(buf[:, :T].cpu().numpy(), s)


# ---- 4. rows shorter than the orders, no future, one lane ----------------------------------------------------------
@pytest.mark.parametrize("order", X.SHORT_ORDERS, ids=X.order_id)
def test_short_forecasts_match_oracle(engine, order):
    p, d, q, I = order
    s, coef = X.short_inputs(order)
    exp = X.short_expect(order)
    for (T, nf), e in exp.items():
        for N in X.SHORT_N:
            out = engine.forecast(s[:N, :T], p, d, q, I, coef[:N], nf)
            assert out.shape == (N, T + nf)
            assert _same(out, e[:N]), (order, T, nf, N)


def test_forecast_d_17_is_refused(engine):
    import torch
    N, T, nf = 4, 40, 3
    s = np.random.default_rng(17).standard_normal((N, T))
    coef = np.full((N, 2), 0.1)
    with pytest.raises(L.EngineError):
        engine.forecast(s, 1, 17, 1, 0, coef, nf)
    buf, dcoef = torch.tensor(s, device="cuda"), torch.tensor(coef, device="cuda")
    dout = torch.full((N, T + nf), -7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(L.EngineError):
        engine.forecast_device(buf.data_ptr(), N, T, T, 1, 17, 1, 0, dcoef.data_ptr(), nf, dout.data_ptr(), T + nf)
    engine.synchronize()
    assert torch.all(dout == -7.0)                           # a refused call writes nothing
    out = engine.forecast(s, 1, 16, 1, 0, coef, nf)          # the ceiling itself is served
    assert _same(out, np.stack([O.forecast(s[i], 1, 16, 1, 0, coef[i], nf) for i in range(N)]))


# ---- 5. the maximum orders and the dispatch boundary ---------------------------------------------------------------
@pytest.mark.parametrize("pq", X.BLOCK_PQ, ids=lambda pq: f"{pq[0]}_{pq[1]}")
def test_max_order_gradient_loglik_flags(engine, pq):
    p, q = pq
    y, coefs = X.block_inputs(pq)
    exp = X.block_expect(pq)
    for I in (0, 1):
        c, wide = coefs[I]
        for smear in (0, 1):
            engine.set_option("smear", smear)
            try:
                g = engine.css_gradient(y, p, q, I, c)
            finally:
                engine.set_option("smear", L.DEFAULT_SMEAR)
            assert _same(g, exp[I]["grad"][smear]), (pq, I, smear)
        assert _same(engine.css_loglik(y, p, 0, q, I, c), exp[I]["ll"]), (pq, I)
        assert np.array_equal(engine.model_flags(c, p, q, I), exp[I]["flags"]), (pq, I)
        assert np.array_equal(engine.model_flags(wide, p, q, I), exp[I]["wide_flags"]), (pq, I)


def test_max_order_hannan_rissanen(engine):
    p, q, I = X.HR_MAX
    for y, (est, eini) in zip(X.hr_max_inputs(), X.hr_max_expect()):     # T = 200; 82 (41 x 41, square); 83
        init, st = engine.hannan_rissanen(y, p, q, I)
        assert np.array_equal(st, est), y.shape
        assert _same(init, eini), y.shape


@pytest.mark.parametrize("case", X.FIT_CASES, ids=X.fit_case_id)
def test_max_order_and_boundary_fits(engine, case):
    p, d, q, I, smear = case
    rows, exp = X.fit_case(case)
    engine.set_option("smear", smear)
    try:
        res = engine.fit_batch(rows, p, d, q, bool(I))
        st = engine.stats()
    finally:
        engine.set_option("smear", L.DEFAULT_SMEAR)
    check_fit(res, exp, f"ARIMA{case[:4]} smear={smear}")
    assert st["series_done"] == len(rows) and st["n_eval"] == int(res["n_eval"].sum())


# ---- 6. special values beside clean rows ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", X.SPECIAL_ORDERS, ids=X.order_id)
def test_special_values_in_one_wave(engine, order):
    p, d, q, I = order
    rows, exp = X.special_rows(order), X.special_expect(order)
    res = engine.fit_batch(rows, p, d, q, bool(I))
    check_fit(res, exp, f"ARIMA{order} special rows")        # NaN positions of normal returns included
    for i in X.SPECIAL_CLEAN:                                # a bad neighbour changes nothing in a clean row's fit
        one = engine.fit_batch(rows[i:i + 1], p, d, q, bool(I))
        for k in ("status", "n_eval", "n_grad", "flags"):
            assert one[k][0] == res[k][i], (k, i)
        assert _same(one["coef"][0], res["coef"][i]) and _same(one["ll"][0], res["ll"][i]), i


# ---- 7. null optional outputs; css-bobyqa's last dimension ---------------------------------------------------------
def test_device_entry_with_null_optional_outputs(engine):
    import torch
    p, d, q, I = X.NULLS_ORDER
    N, T = X.NULLS_N, X.NULLS_T
    k = p + q + I
    buf = torch.tensor(X.nulls_rows(), device="cuda")

    def outputs():
        return [torch.full((N, k), -7.0, dtype=torch.float64, device="cuda"),
                torch.full((N,), -7.0, dtype=torch.float64, device="cuda"),
                torch.full((N,), -7, dtype=torch.int32, device="cuda")]

    full = outputs() + [torch.full((N,), -7, dtype=torch.int32, device="cuda") for _ in range(2)] + \
        [torch.full((N,), 77, dtype=torch.uint8, device="cuda")]
    engine.fit_batch_device(buf.data_ptr(), N, T, T, p, d, q, I, *[t.data_ptr() for t in full])
    f = [t.cpu().numpy() for t in full]
    check_fit(dict(coef=f[0], ll=f[1], status=f[2], n_eval=f[3], n_grad=f[4], flags=f[5]), X.nulls_expect(),
              "device entry, every output")
    some = outputs()
    engine.fit_batch_device(buf.data_ptr(), N, T, T, p, d, q, I, *[t.data_ptr() for t in some])   # the rest: None
    st = engine.stats()
    for a, b in zip(some, f):
        assert _same(a.cpu().numpy(), b)
    assert st["series_done"] == N and st["n_eval"] == int(f[3].sum())


def test_css_bobyqa_at_its_last_dimension(engine):
    p, d, q, I = X.BOBYQA_LAST
    rows = X.bobyqa_rows()
    res = engine.fit_batch(rows, p, d, q, bool(I), method="css-bobyqa")
    check_fit(res, X.bobyqa_expect(), "css-bobyqa (6,0,4)+c")
    p, d, q, I = X.BOBYQA_REFUSED
    with pytest.raises(L.EngineError):                       # 12 parameters: one past the compiled dimensions
        engine.fit_batch(rows, p, d, q, bool(I), method="css-bobyqa")
