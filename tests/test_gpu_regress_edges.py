"""The regression kernels (csrc/arima_regress.hip) at the edges tests/test_gpu_regress.py never reaches: the assembly's
32-row tiles and a lag longer than a tile, the prediction's 16-row chunks, the widest design (64 columns, 32 KiB of
dynamic LDS), several slices under padded strides, the shape statuses without an intercept, and special values in
bgtest and bptest. Everything is held to tests/regress_ref.py exactly as there: coefficients, predictions and statistics
bit for bit, the statuses equal, the p-values to P_TOL.

Unless a test says otherwise the calls go through the device entry points with a row stride of T + 3 and a per-series
regressor stride of k T + 5, NaN in every gap, outputs pre-filled with a sentinel and followed by guard elements, and a
prediction stride of R + 3: a read or a write one element out of place shows."""
import numpy as np
import pytest

import regress_ref as R
import sparkts_amd._lib as L
from test_gpu_diag import P_TOL, _p_close, _same
from test_gpu_regress import CONFIGS, _arx_case, _ref_fit, _ref_predict

pytestmark = pytest.mark.gpu

SENT, ISENT, GUARD = -7.0, -7, 8
_memo = {}


def memo(key, make):
    """References are computed once, shared among the tests and left unchanged."""
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


# ---- the device entry points under padded strides ---------------------------------------------------------------------
class Src:
    """y (N, T) with row stride T + 3 and x on the device: x (N, T, k) per series, k rows of T values each, k T + 5
    apart; x (T, k) one matrix shared by every series (x_series_stride 0). NaN in every gap."""

    def __init__(self, y, x):
        import torch
        y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
        self.N, self.T = y.shape
        self.ld, self.k = self.T + 3, x.shape[-1]
        host = np.full((self.N, self.ld), np.nan)
        host[:, :self.T] = y
        self.y = torch.from_numpy(host).cuda()
        if x.ndim == 2:
            self.xs = 0
            self.x = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
        else:
            self.xs = self.k * self.T + 5
            xh = np.full((self.N, self.xs), np.nan)
            xh[:, :self.k * self.T] = x.transpose(0, 2, 1).reshape(self.N, self.k * self.T)
            self.x = torch.from_numpy(xh).cuda()

    def args(self):
        return self.y.data_ptr(), self.N, self.T, self.ld, self.x.data_ptr(), self.xs, self.k


def _out(n, dtype="float64"):
    import torch
    return torch.full((n + GUARD,), SENT if dtype == "float64" else ISENT, dtype=getattr(torch, dtype), device="cuda")


def _body(t, n, what):
    a = t.cpu().numpy()
    assert np.all(a[n:] == (SENT if a.dtype.kind == "f" else ISENT)), f"{what}: written past the output"
    return a[:n]


def dev_fit(engine, src, yl, xl, orig, noint):
    K = engine.arx_num_coef(src.k, yl, xl, orig)
    coef, status = _out(src.N * (1 + K)), _out(src.N, "int32")
    engine.arx_fit_device(*src.args(), yl, xl, orig, noint, coef.data_ptr(), status.data_ptr())
    return dict(coef=_body(coef, src.N * (1 + K), "coef").reshape(src.N, 1 + K), status=_body(status, src.N, "status"))


def dev_predict(engine, src, yl, xl, orig, coef, expect=L.ARIMA_OK):
    """(N, R) predictions written with a row stride of R + 3 into a sentinel-filled buffer with a guard row."""
    import torch
    Rr = max(src.T - max(yl, xl), 0)
    cd = torch.from_numpy(np.ascontiguousarray(coef, dtype=np.float64)).cuda()
    out = torch.full((src.N + 1, Rr + 3), SENT, dtype=torch.float64, device="cuda")
    rc = engine.L.arima_arx_predict_batch_device(engine.h, *src.args(), yl, xl, int(orig), cd.data_ptr(),
                                                 out.data_ptr(), Rr + 3, None)
    assert rc == expect, engine.L.arima_last_error(engine.h)
    engine.synchronize()
    o = out.cpu().numpy()
    assert np.all(o[:, Rr:] == SENT) and np.all(o[src.N] == SENT), "written past a prediction row"
    return o[:src.N, :Rr]


def dev_test(engine, which, src, *lag):
    stat, pv, status = _out(src.N), _out(src.N), _out(src.N, "int32")
    run = engine.bgtest_device if which == "bg" else engine.bptest_device
    run(*src.args(), *lag, stat.data_ptr(), pv.data_ptr(), status.data_ptr())
    return dict(stat=_body(stat, src.N, "stat"), pvalue=_body(pv, src.N, "pvalue"),
                status=_body(status, src.N, "status"))


def _ref_test(which, u, f, *lag):
    """regress_ref over the rows of u (N, T) and f (N, T, k): dict(stat, pvalue, status)."""
    ref = [R.bgtest(u[i], f[i].T, *lag) if which == "bg" else R.bptest(u[i], f[i].T) for i in range(len(u))]
    return dict(status=np.array([r[0] for r in ref], dtype=np.int32), stat=np.array([r[1] for r in ref]),
                pvalue=np.array([r[2] for r in ref]))


def _check_fit(got, coef, status, what):
    assert np.array_equal(got["status"], status), (what, got["status"], status)
    assert _same(got["coef"], coef), what
    assert np.all(np.isnan(got["coef"][status != R.ST_OK])), what


def _check_test(got, ref, what):
    assert np.array_equal(got["status"], ref["status"]), (what, got["status"], ref["status"])
    assert _same(got["stat"], ref["stat"]), what
    assert _p_close(got["pvalue"], ref["pvalue"]), (what, P_TOL)


def _series(seed, N, T, k):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, T, k))
    y = np.cumsum(rng.standard_normal((N, T)), axis=1) * 0.3 + x.sum(axis=2) + 2.0
    return y, x


def _head(ref, N):
    return {key: v[:N] for key, v in ref.items()}


def _per_series(x, N):
    return np.ascontiguousarray(np.broadcast_to(x, (N,) + x.shape))


# ---- 1. assembly tile edges -------------------------------------------------------------------------------------------
TILE_T = [31, 32, 33, 63, 64, 65, 97]           # RowTile<32>: one tile short, exact, one over; two; three and a row
TILE_CFG = (3, 2, 2, True, False)               # windows at offsets 0 .. 3: every tile boundary is straddled
TILE_LAG = 4                                    # bgtest's max_lag


def _tile_case(T):
    def make():
        yl, xl, k, orig, noint = TILE_CFG
        y, x = _series(3000 + T, 65, T, k)
        coef, status = _ref_fit(y, x, yl, xl, orig, noint)
        return dict(y=y, x=x, coef=coef, status=status, pred=_ref_predict(y, x, coef, yl, xl, orig),
                    bg=_ref_test("bg", y, x, TILE_LAG), bp=_ref_test("bp", y, x))
    return memo(("tile", T), make)


@pytest.mark.parametrize("N", [1, 64, 65])
@pytest.mark.parametrize("T", TILE_T)
def test_assembly_tile_edges(engine, T, N):
    yl, xl, k, orig, noint = TILE_CFG
    c = _tile_case(T)
    assert np.all(c["status"] == R.ST_OK)
    src = Src(c["y"][:N], c["x"][:N])
    got = dev_fit(engine, src, yl, xl, orig, noint)
    _check_fit(got, c["coef"][:N], c["status"][:N], ("arx", T, N))
    assert _same(dev_predict(engine, src, yl, xl, orig, got["coef"]), c["pred"][:N]), ("predict", T, N)
    _check_test(dev_test(engine, "bg", src, TILE_LAG), _head(c["bg"], N), ("bgtest", T, N))
    _check_test(dev_test(engine, "bp", src), _head(c["bp"], N), ("bptest", T, N))


@pytest.mark.parametrize("T", [31, 32, 33, 65])
def test_assembly_tile_edges_shared_x(engine, T):
    # a shared matrix is read directly, not through the tile: held to the same matrix given per series and to the
    # restatement
    yl, xl, k, orig, noint = TILE_CFG
    N = 65
    y = _tile_case(T)["y"]
    x = np.random.default_rng(3500 + T).standard_normal((T, k))

    def make():
        per = _per_series(x, N)
        coef, status = _ref_fit(y, per, yl, xl, orig, noint)
        return dict(coef=coef, status=status, pred=_ref_predict(y, per, coef, yl, xl, orig),
                    bg=_ref_test("bg", y, per, TILE_LAG), bp=_ref_test("bp", y, per))
    ref = memo(("tile_shared", T), make)
    shared, per = Src(y, x), Src(y, _per_series(x, N))
    assert shared.xs == 0 and per.xs == k * T + 5
    fits = [dev_fit(engine, s, yl, xl, orig, noint) for s in (shared, per)]
    for got in fits:
        _check_fit(got, ref["coef"], ref["status"], ("arx", T))
    for s in (shared, per):
        assert _same(dev_predict(engine, s, yl, xl, orig, fits[0]["coef"]), ref["pred"]), ("predict", T)
        _check_test(dev_test(engine, "bg", s, TILE_LAG), ref["bg"], ("bgtest", T))
        _check_test(dev_test(engine, "bp", s), ref["bp"], ("bptest", T))
    a, b = dev_test(engine, "bg", shared, TILE_LAG), dev_test(engine, "bg", per, TILE_LAG)
    assert _same(a["pvalue"], b["pvalue"])                       # the same statistic through the same code: the same bits


# ---- 2. a lag longer than a tile --------------------------------------------------------------------------------------
LONG_T, LONG_N = 97, 65


def _long_case():
    return memo("long", lambda: _series(4000, LONG_N, LONG_T, 1))


def test_y_lag_longer_than_a_tile(engine):
    # C = 35, R = 64, column offsets 0 .. 33: the oldest lag's window ends before the last tile begins, the newest
    # columns' windows begin after the first tile
    y, x = _long_case()
    coef, status = memo("long_y", lambda: _ref_fit(y, x, 33, 0, True, False))
    assert coef.shape == (LONG_N, 35) and np.all(status == R.ST_OK)
    src = Src(y, x)
    got = dev_fit(engine, src, 33, 0, True, False)
    _check_fit(got, coef, status, "yMaxLag 33")
    pred = memo("long_y_pred", lambda: _ref_predict(y, x, coef, 33, 0, True))
    assert pred.shape == (LONG_N, 64) and _same(dev_predict(engine, src, 33, 0, True, got["coef"]), pred)


@pytest.mark.parametrize("shared", [False, True], ids=["per_series_x", "shared_x"])
def test_x_lag_longer_than_a_tile(engine, shared):
    y, x = _long_case()
    xm = x[0] if shared else x                                   # (T, 1): one matrix for every series
    per = _per_series(xm, LONG_N) if shared else x
    coef, status = memo(("long_x", shared), lambda: _ref_fit(y, per, 0, 34, False, False))
    assert coef.shape == (LONG_N, 35) and np.all(status == R.ST_OK)
    src = Src(y, xm)
    got = dev_fit(engine, src, 0, 34, False, False)
    _check_fit(got, coef, status, ("xMaxLag 34", shared))
    pred = memo(("long_x_pred", shared), lambda: _ref_predict(y, per, coef, 0, 34, False))
    assert _same(dev_predict(engine, src, 0, 34, False, got["coef"]), pred)


def test_bgtest_lag_longer_than_a_tile(engine):
    y, x = _long_case()
    ref = memo("long_bg", lambda: _ref_test("bg", y, x, 33))
    assert np.all(ref["status"] == R.ST_OK)
    _check_test(dev_test(engine, "bg", Src(y, x), 33), ref, "bgtest max_lag 33")


# ---- 3. predict chunk edges -------------------------------------------------------------------------------------------
PRED_CFG = (2, 1, 2, True)                      # maxLag 2, K = 2 + 2 + 2
PRED_R = [0, 1, 15, 16, 17, 32, 33]             # kRgPredCH = 16: none, one row, a chunk less one, exact, one over, two ...


def _pred_case(Rr):
    def make():
        yl, xl, k, orig = PRED_CFG
        y, x = _series(5000 + Rr, 65, Rr + 2, k)
        coef = np.random.default_rng(5100 + Rr).uniform(-1.5, 1.5, (65, 1 + 6))
        return y, x, coef, np.array(_ref_predict(y, x, coef, yl, xl, orig)).reshape(65, Rr)
    return memo(("pred", Rr), make)


@pytest.mark.parametrize("N", [1, 65])
@pytest.mark.parametrize("Rr", PRED_R)
def test_predict_chunk_edges(engine, Rr, N):
    yl, xl, k, orig = PRED_CFG
    y, x, coef, pred = (a[:N] for a in _pred_case(Rr))
    got = dev_predict(engine, Src(y, x), yl, xl, orig, coef)     # R = 0: ARIMA_OK, and every sentinel is still there
    assert got.shape == (N, Rr) and _same(got, pred), (Rr, N)


def test_predict_special_values(engine):
    yl, xl, k, orig = PRED_CFG
    y, x, coef, _ = (a.copy() for a in _pred_case(33))
    coef[1, 0] = np.nan                                          # c
    coef[2, 3] = np.inf
    coef[63, 6] = -np.inf
    coef[64, 1] = np.nan
    coef[5, 2] = 0.0                                             # 0 * Inf below
    y[3, 17] = np.nan
    y[4, 0] = np.inf                                             # only ever a lagged value
    y[5, 20] = -np.inf
    x[6, 34, 1] = np.nan                                         # the last row's own x
    x[64, 16, 0] = np.inf
    pred = np.array(_ref_predict(y, x, coef, yl, xl, orig))
    assert np.all(np.isnan(pred[1])) and np.isnan(pred[5]).any() and not np.isnan(pred[7:63]).any()
    assert _same(dev_predict(engine, Src(y, x), yl, xl, orig, coef), pred)


# ---- 4. the widest design: 64 columns, 32 KiB of dynamic LDS in k_regress_qr and k_regress_r2 -----------------------
WIDE_N = 65


@pytest.mark.parametrize("T,yl,noint", [(141, 61, False), (142, 62, True)], ids=["intercept", "no_intercept"])
def test_widest_arx_design_fits(engine, T, yl, noint):
    y, x = memo(("wide_arx", T), lambda: _series(6000 + T, WIDE_N, T, 2))
    coef, status = memo(("wide_arx_ref", T), lambda: _ref_fit(y, x, yl, 0, True, noint))
    assert np.all(status == R.ST_OK) and coef.shape == (WIDE_N, 1 + yl + 2)       # 64 columns, R = 80
    assert (yl + 2) + (0 if noint else 1) == 64
    src = Src(y, x)
    got = dev_fit(engine, src, yl, 0, True, noint)
    _check_fit(got, coef, status, ("widest arx", T))
    if noint:
        assert np.all(got["coef"][:, 0] == 0.0)
    pred = memo(("wide_arx_pred", T), lambda: _ref_predict(y, x, coef, yl, 0, True))
    assert _same(dev_predict(engine, src, yl, 0, True, got["coef"]), pred)


def test_widest_bgtest_design(engine):
    u, f = memo("wide_bg", lambda: _series(6300, WIDE_N, 140, 3))                 # 1 + 3 + 60 columns, df = 60
    ref = memo("wide_bg_ref", lambda: _ref_test("bg", u, f, 60))
    assert np.all(ref["status"] == R.ST_OK)
    _check_test(dev_test(engine, "bg", Src(u, f), 60), ref, "bgtest max_lag 60")


def test_widest_bptest_design(engine):
    u, f = memo("wide_bp", lambda: _series(6400, WIDE_N, 100, 63))                # 1 + 63 columns, df = 63
    ref = memo("wide_bp_ref", lambda: _ref_test("bp", u, f))
    assert np.all(ref["status"] == R.ST_OK)
    _check_test(dev_test(engine, "bp", Src(u, f)), ref, "bptest k 63")


def test_65_columns_stay_unsupported(engine):
    y, x = memo(("wide_arx", 142), lambda: _series(6000 + 142, WIDE_N, 142, 2))
    src = Src(y, x)
    coef, status = _out(WIDE_N * 65), _out(WIDE_N, "int32")
    rc = engine.L.arima_arx_fit_batch_device(engine.h, *src.args(), 62, 0, 1, 0, coef.data_ptr(), status.data_ptr(),
                                             None)
    assert rc == L.ARIMA_E_UNSUPPORTED and engine.L.arima_last_error(engine.h) == b"at most 64 columns"
    engine.synchronize()
    _body(coef, 0, "coef of a refused call")
    _body(status, 0, "status of a refused call")


# ---- 5. several slices under padded strides ---------------------------------------------------------------------------
def test_slices_under_padded_strides(engine):
    cfg = CONFIGS[5]                                             # (3, 2, 3, True, intercept), T = 40
    yl, xl, k, orig, noint = cfg
    N = 130
    y, x0, coef0, status0, _ = _arx_case(cfg)
    x = x0.copy()
    x[64, :, 1] = 0.0                                            # SINGULAR: the first row of the second slice
    x[129, :, 2] = 0.0                                           # ... and the last row of the partial slice

    def make():
        coef, status = coef0.copy(), status0.copy()
        coef[[64, 129]], status[[64, 129]] = _ref_fit(y[[64, 129]], x[[64, 129]], yl, xl, orig, noint)
        return dict(coef=coef, status=status, pred=_ref_predict(y, x, coef, yl, xl, orig),
                    bg=_ref_test("bg", y, x, 2), bp=_ref_test("bp", y, x))
    ref = memo("slices", make)
    assert ref["status"][64] == ref["status"][129] == R.ST_SINGULAR and np.sum(ref["status"] != R.ST_OK) == 2
    assert ref["bg"]["status"][64] == ref["bp"]["status"][129] == R.ST_SINGULAR
    src = Src(y, x)

    def run():
        fit = dev_fit(engine, src, yl, xl, orig, noint)
        return (fit, dev_predict(engine, src, yl, xl, orig, fit["coef"]), dev_test(engine, "bg", src, 2),
                dev_test(engine, "bp", src))
    whole = run()
    before = engine.get_option("regress_slice_bytes")
    assert before == 0
    engine.set_option("regress_slice_bytes", 1)                  # one block of 64 series per slice: 64 + 64 + 2
    try:
        sliced = run()
    finally:
        engine.set_option("regress_slice_bytes", before)
    for fit, pred, bg, bp in (whole, sliced):
        _check_fit(fit, ref["coef"], ref["status"], "slices: arx")
        assert _same(pred, ref["pred"]), "slices: predict"
        _check_test(bg, ref["bg"], "slices: bgtest")
        _check_test(bp, ref["bp"], "slices: bptest")
    for a, b in zip(whole[2:], sliced[2:]):
        assert _same(a["pvalue"], b["pvalue"])                   # one slice or three: the same bits


# ---- 6. shape statuses without an intercept ---------------------------------------------------------------------------
@pytest.mark.parametrize("T,want", [(8, R.ST_NOT_ENOUGH_DATA),   # R = 6 = K: validateSampleData refuses it here too
                                    (9, R.ST_OK), (2, R.ST_NO_DATA), (1, R.ST_SERIES_TOO_SHORT)])
def test_shape_statuses_without_an_intercept(engine, T, want):
    yl, xl, k, orig, noint = 2, 1, 2, True, True                 # K = 6
    N = 66
    y, x = _series(7000 + T, N, T, k)
    coef, status = _ref_fit(y, x, yl, xl, orig, noint)
    assert np.all(status == want) and coef.shape == (N, 7)
    got = dev_fit(engine, Src(y, x), yl, xl, orig, noint)
    _check_fit(got, coef, status, ("no intercept", T))
    if want == R.ST_OK:
        assert np.all(got["coef"][:, 0] == 0.0) and not np.any(np.isnan(got["coef"]))
    else:
        assert np.all(np.isnan(got["coef"]))


# ---- 7. special values in bgtest and bptest ---------------------------------------------------------------------------
SPECIAL_ROWS = [0, 63, 64, 69]                  # the first lane, the last lane of a block, the next block's first, the last


def _special_base():
    def make():
        rng = np.random.default_rng(8000)
        u, f = rng.standard_normal((70, 20)), rng.standard_normal((70, 20, 2))
        return u, f, _ref_test("bg", u, f, 2), _ref_test("bp", u, f)
    return memo("special", make)


def _constant(u, f):
    u[:] = 3.25


def _zero(u, f):
    u[:] = 0.0


def _nan_in_u(u, f):
    u[11] = np.nan


def _inf_in_u(u, f):
    u[7] = np.inf


def _nan_in_factor(u, f):
    f[5, 1] = np.nan


@pytest.mark.parametrize("spoil", [_constant, _zero, _nan_in_u, _inf_in_u, _nan_in_factor], ids=lambda f: f.__name__[1:])
def test_special_values_in_the_tests(engine, spoil):
    u0, f0, bg0, bp0 = _special_base()
    u, f = u0.copy(), f0.copy()
    for i in SPECIAL_ROWS:
        spoil(u[i], f[i])
    ordinary = np.ones(70, dtype=bool)
    ordinary[SPECIAL_ROWS] = False
    src, base = Src(u, f), Src(u0, f0)
    for which, lag, ref0 in (("bg", (2,), bg0), ("bp", (), bp0)):
        ref = {key: v.copy() for key, v in ref0.items()}
        sp = _ref_test(which, u[SPECIAL_ROWS], f[SPECIAL_ROWS], *lag)
        for key in ref:
            ref[key][SPECIAL_ROWS] = sp[key]
        got = dev_test(engine, which, src, *lag)
        _check_test(got, ref, (which, spoil.__name__))
        clean = memo(("special_dev", which), lambda: dev_test(engine, which, base, *lag))
        _check_test(clean, ref0, (which, "no special rows"))
        for key in got:                                          # the neighbours of a special row: the bits of a batch without
            assert _same(got[key][ordinary], clean[key][ordinary]), (which, spoil.__name__, key)
        if which == "bp":
            # what the restatement gives today, so that a change of the restatement cannot silently move it
            st, stat, pv = (got[key][SPECIAL_ROWS] for key in ("status", "stat", "pvalue"))
            assert np.all(st == R.ST_OK)
            if spoil is _constant:                               # TSS = 0, RSS > 0 by rounding: R^2 = -inf
                assert np.all(stat == -np.inf) and np.all(pv == 1.0)
            else:
                assert np.all(np.isnan(stat)) and np.all(np.isnan(pv))
        elif spoil in (_nan_in_u, _inf_in_u, _nan_in_factor):    # the JVM goes on: status OK, NaN out
            assert np.all(got["status"][SPECIAL_ROWS] == R.ST_OK) and np.all(np.isnan(got["stat"][SPECIAL_ROWS]))
