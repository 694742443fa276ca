"""Batched residual diagnostics on the device (csrc/arima_diag.hip) against the CPU restatement tests/diag_ref.py:
autocorr, dwtest and the Ljung-Box statistic bit for bit (NaNs in the same places), the p-value to P_TOL."""
import ctypes

import numpy as np
import pytest

import diag_ref as R
import sparkts_amd._lib as L
from test_diag_ref import jni_diag

pytestmark = pytest.mark.gpu

ARIMA_E_INVALID_ARG = -1
W = 8                                   # lags per group of the kernel (kDgW, csrc/arima_launch.hpp)
# 4 x the largest |restated p - torch.special.gammaincc| over L = 1..40, stat in [1e-3, 300] (5.773e-15, printed by
# tests/test_diag_ref.py::test_pvalue_restatement_against_torch_gammaincc), never above that test's cap
P_TOL = min(4 * 5.773e-15, 1e-10)
SENT = -7.0


def _same(a, b):
    """Bit for bit, NaNs in the same places (a NaN's sign and payload are not compared)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def _p_close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.all(np.abs(a[~na] - b[~nb]) <= P_TOL))


def _ref(rows, max_lag, acf_full=None):
    """The restatement's four outputs; acf_full: the rows' autocorr at some larger lag count (every lag is its own
    computation, so fewer lags are its leading columns)."""
    rows = np.atleast_2d(rows)
    acf = [R.autocorr(r, max_lag) for r in rows] if acf_full is None else [list(a[:max_lag]) for a in acf_full]
    dw = [R.dwtest(r) for r in rows]
    st = [R.lb_stat_from_acf(a, rows.shape[1]) for a in acf]
    pv = [R.chisq_upper_tail(max_lag, s) for s in st]
    return np.array(acf).reshape(len(rows), max_lag), np.array(dw), np.array(st), np.array(pv)


def _check(got, exp, what=""):
    acf, dw, st, pv = exp
    assert _same(got["acf"], acf), f"acf {what}"
    assert _same(got["dw"], dw), f"dw {what}"
    assert _same(got["lb_stat"], st), f"lb_stat {what}"
    assert _p_close(got["lb_pvalue"], pv), f"lb_pvalue {what}: {np.nanmax(np.abs(got['lb_pvalue'] - pv))}"


# ---- 1. bit parity with the restatement ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parity_rows():
    rng = np.random.default_rng(20261019)
    N, T = 96, 211
    rows = rng.standard_normal((N, T))
    rows[:48] = np.cumsum(rows[:48], axis=1)                       # random walks, then white noise
    return rows, [R.autocorr(r, 40) for r in rows]


@pytest.mark.parametrize("max_lag", [1, 2, 3, 4, W - 1, W, W + 1, 2 * W + 1, 40])   # 2, 3, 4: the narrower instances
def test_diag_bit_parity(engine, parity_rows, max_lag):
    rows, acf40 = parity_rows
    _check(engine.diagnostics(rows, max_lag), _ref(rows, max_lag, acf40), f"max_lag {max_lag}")


# ---- 2. tile and group edges through the device entry points --------------------------------------------------------
_EDGE_REF = {}


def _edge_ref(T):
    if T not in _EDGE_REF:
        rng = np.random.default_rng(T)
        rows = np.cumsum(rng.standard_normal((65, T)), axis=1)
        _EDGE_REF[T] = rows, [R.autocorr(r, T - 1) for r in rows]
    return _EDGE_REF[T]


@pytest.mark.parametrize("N", [1, 64, 65])
@pytest.mark.parametrize("T", [2, 31, 32, 33, 65])
def test_diag_tile_and_group_edges(engine, T, N):
    import torch
    rows65, acf_full = _edge_ref(T)
    rows = rows65[:N]
    ld, pad = T + 8, 24
    host = np.full((N, ld), np.nan)                                # padding columns must never be consumed
    host[:, :T] = rows
    sd = torch.from_numpy(host).cuda()
    for max_lag in sorted({1, min(W + 1, T - 1), T - 1}):
        acf = torch.full((N * max_lag + pad,), SENT, dtype=torch.float64, device="cuda")
        vec = [torch.full((N + pad,), SENT, dtype=torch.float64, device="cuda") for _ in range(3)]
        engine.diagnostics_device(sd.data_ptr(), N, T, ld, max_lag, acf.data_ptr(), vec[0].data_ptr(),
                                  vec[1].data_ptr(), vec[2].data_ptr())
        a, v = acf.cpu().numpy(), [x.cpu().numpy() for x in vec]
        assert np.all(a[N * max_lag:] == SENT) and all(np.all(x[N:] == SENT) for x in v), "written past the outputs"
        got = {"acf": a[:N * max_lag].reshape(N, max_lag), "dw": v[0][:N], "lb_stat": v[1][:N], "lb_pvalue": v[2][:N]}
        _check(got, _ref(rows, max_lag, acf_full[:N]), f"T {T} N {N} max_lag {max_lag}")
        if T == 2:
            assert np.all(np.isnan(got["acf"]))                    # T - lag == 1: 0 / 0


# ---- 3. special values ---------------------------------------------------------------------------------------------
def test_diag_special_values(engine):
    rng = np.random.default_rng(7)
    T = 64
    rows = rng.standard_normal((6, T))
    rows[0] = 3.25                                                 # constant: NaN correlations, dw = 0 / sum r^2
    rows[1, 17] = np.nan
    rows[2, 40] = np.inf
    rows[3, 5] = -np.inf
    rows[4] = 0.0                                                  # dw = 0 / 0
    for max_lag in (3, W + 1):
        got = engine.diagnostics(rows, max_lag)
        _check(got, _ref(rows, max_lag), f"max_lag {max_lag}")
        assert np.all(np.isnan(got["acf"][:5])) and got["dw"][0] == 0.0 and np.isnan(got["dw"][4])
        assert not np.any(np.isnan(got["acf"][5]))
    one = np.array([[2.0], [0.0], [np.nan]])                       # T = 1: only dwtest is defined
    dw = engine.diagnostics(one, 0, ("dw",))["dw"]
    assert _same(dw, [R.dwtest(r) for r in one]) and dw[0] == 0.0 and np.isnan(dw[1])


# ---- 4. the Int product n * (n + 2) wraps on the device as in the JVM ------------------------------------------------
@pytest.mark.parametrize("T", [46339, 46340])
def test_diag_int_wrap(engine, T):
    rng = np.random.default_rng(T)
    rows = np.cumsum(rng.standard_normal((2, T)), axis=1)
    got = engine.diagnostics(rows, 1)
    exp = _ref(rows, 1)
    _check(got, exp, f"T {T}")
    if T < 46340:
        assert np.all(got["lb_stat"] > 0)
    else:
        assert np.all(got["lb_stat"] < 0) and np.all(got["lb_pvalue"] == 1.0)


# ---- 5. nullable outputs and refusals --------------------------------------------------------------------------------
def test_diag_single_outputs_equal_the_full_call(engine):
    rng = np.random.default_rng(11)
    rows = np.cumsum(rng.standard_normal((70, 50)), axis=1)
    for max_lag in (5, 12):
        full = engine.diagnostics(rows, max_lag)
        for name in L.Engine.DIAG_OUTPUTS:
            alone = engine.diagnostics(rows, max_lag, (name,))
            assert list(alone) == [name] and _same(alone[name], full[name]), (name, max_lag)


def test_diag_refusals_write_nothing(engine):
    import torch
    N, T, ld = 5, 20, 24
    buf = torch.full((N * ld + 4 * N * T,), SENT, dtype=torch.float64, device="cuda")
    base = buf.data_ptr()
    out = [base + (N * ld + j * N * T) * 8 for j in range(4)]
    abi = engine.L.arima_diagnostics_batch_device
    assert abi(engine.h, base, N, T, ld, 0, out[0], None, None, None, None) == ARIMA_E_INVALID_ARG      # max_lag 0
    assert abi(engine.h, base, N, T, ld, 0, None, None, out[2], None, None) == ARIMA_E_INVALID_ARG
    assert abi(engine.h, base, N, T, ld, T, out[0], out[1], out[2], out[3], None) == ARIMA_E_INVALID_ARG  # max_lag T
    assert abi(engine.h, base, N, T, T - 1, 3, out[0], out[1], out[2], out[3], None) == ARIMA_E_INVALID_ARG  # ld < T
    last = base + 8 * ((N - 1) * ld + T - 1)                       # the rows' last element
    assert abi(engine.h, base, N, T, ld, 3, last, None, None, None, None) == ARIMA_E_INVALID_ARG            # acf on the rows
    assert abi(engine.h, base, N, T, ld, 3, None, base, None, None, None) == ARIMA_E_INVALID_ARG        # dw on the rows
    assert abi(engine.h, base, N, T, ld, 3, out[0], out[0] + 8, None, None, None) == ARIMA_E_INVALID_ARG  # out on out
    assert abi(engine.h, base, 0, T, ld, 3, out[0], out[1], out[2], out[3], None) == 0                  # N == 0
    assert abi(engine.h, base, N, 0, ld, 3, out[0], out[1], out[2], out[3], None) == 0                  # T == 0
    assert abi(engine.h, base, N, T, ld, -4, None, out[1], None, None, None) == 0                       # dw alone
    engine.synchronize()
    got = buf.cpu().numpy()
    dw = got[N * ld + N * T:N * ld + N * T + N]
    assert _same(dw, [R.dwtest([SENT] * T)] * N)                                                         # the one call that ran
    got[N * ld + N * T:N * ld + N * T + N] = SENT
    assert np.all(got == SENT)
    host = engine.L.arima_diagnostics_batch
    x, o = np.zeros((N, T)), np.full((N, 3), SENT)
    dp = ctypes.POINTER(ctypes.c_double)
    assert host(engine.h, x.ctypes.data_as(dp), N, T, T, o.ctypes.data_as(dp), None, None, None) == ARIMA_E_INVALID_ARG
    assert host(engine.h, x.ctypes.data_as(dp), N, T, 3, x.ctypes.data_as(dp), None, None, None) == ARIMA_E_INVALID_ARG
    assert np.all(o == SENT) and np.all(x == 0.0)


# ---- 6. diagnostics of residuals without the residuals ---------------------------------------------------------------
@pytest.mark.parametrize("pdq", [(2, 1, 2), (0, 1, 3), (5, 1, 5), (7, 1, 2)])
def test_residual_diagnostics_equal_diagnostics_of_residuals(engine, pdq):
    p, d, q = pdq
    rng = np.random.default_rng(100 * p + q)
    N, T, max_lag = 130, 97, W + 1
    s = np.cumsum(rng.standard_normal((N, T)), axis=1)
    coef = rng.uniform(-0.2, 0.2, (N, 1 + p + q))
    exp = engine.diagnostics(engine.remove_effects(s, p, d, q, True, coef), max_lag)
    got = engine.residual_diagnostics(s, p, d, q, True, coef, max_lag)
    assert all(_same(got[k], exp[k]) for k in L.Engine.DIAG_OUTPUTS)
    few = engine.residual_diagnostics(s, p, d, q, True, coef, W, ("dw", "lb_pvalue"))
    exp_w = engine.diagnostics(engine.remove_effects(s, p, d, q, True, coef), W)
    assert sorted(few) == ["dw", "lb_pvalue"] and all(_same(few[k], exp_w[k]) for k in few)
    assert engine.get_option("diag_slice_bytes") == 0
    try:
        engine.set_option("diag_slice_bytes", 64 * 112 * 8)        # 64 residual rows of stride 112: slices of 64, 64, 2
        sliced = engine.residual_diagnostics(s, p, d, q, True, coef, max_lag)
    finally:
        engine.set_option("diag_slice_bytes", 0)
    assert all(_same(sliced[k], exp[k]) for k in L.Engine.DIAG_OUTPUTS)


def test_residual_diagnostics_device_entry_point(engine):
    import torch
    rng = np.random.default_rng(5)
    N, T, ld, max_lag = 70, 40, 48, 6
    s = np.cumsum(rng.standard_normal((N, T)), axis=1)
    coef = rng.uniform(-0.2, 0.2, (N, 5))
    host = np.full((N, ld), np.nan)
    host[:, :T] = s
    sd, cd = torch.from_numpy(host).cuda(), torch.from_numpy(coef).cuda()
    acf = torch.full((N, max_lag), SENT, dtype=torch.float64, device="cuda")
    pv = torch.full((N,), SENT, dtype=torch.float64, device="cuda")
    engine.residual_diagnostics_device(sd.data_ptr(), N, T, ld, 2, 1, 2, True, cd.data_ptr(), max_lag,
                                       d_acf=acf.data_ptr(), d_lb_pvalue=pv.data_ptr())
    exp = engine.residual_diagnostics(s, 2, 1, 2, True, coef, max_lag)
    assert _same(acf.cpu().numpy(), exp["acf"]) and _same(pv.cpu().numpy(), exp["lb_pvalue"])
    assert torch.equal(sd.cpu()[:, :T], torch.from_numpy(s))                                  # the input is not touched


# ---- 7. the Python mirror ----------------------------------------------------------------------------------------------
def test_fit_result_diagnostics_and_stats_module(engine):
    import torch
    from sparkts_amd import stats
    from sparkts_amd.models import ARIMA
    from sparkts_amd.timeseriesrdd import arima_diagnostics_partition
    N, T = 64, 256
    buf = torch.empty((N, T), dtype=torch.float64, device="cuda")
    engine.sample_device(buf.data_ptr(), N, T, T, 2, 1, 2, 1, [8.2, 0.2, 0.5, 0.3, 0.1], 0.05, 20261019)
    s = buf.cpu().numpy()
    res = ARIMA.fit_models(2, 1, 2, s)
    dg = res.diagnostics(s, 10)
    ok = res.status == L.ST_OK
    assert ok.mean() > 0.9
    exp = engine.residual_diagnostics(s, 2, 1, 2, True, res.coefficients, 10)
    for name, got in (("acf", dg.acf), ("dw", dg.dw), ("lb_stat", dg.lb_stat), ("lb_pvalue", dg.lb_pvalue)):
        assert _same(got[ok], exp[name][ok]) and np.all(np.isnan(got[~ok])), name
    assert dg.acf.shape == (N, 10) and dg.max_lag == 10
    resid = res.residuals(s)[ok][:6]
    acf, dw, st, pv = _ref(resid, 10)
    assert _same(dg.acf[ok][:6], acf) and _same(dg.dw[ok][:6], dw) and _same(dg.lb_stat[ok][:6], st)
    assert _p_close(dg.lb_pvalue[ok][:6], pv)
    rows = resid[:, :60]
    acf, dw, st, pv = _ref(rows, 4)
    assert _same(stats.autocorr(rows, 4), acf) and _same(stats.dwtest(rows), dw)
    got_st, got_pv = stats.lbtest(rows, 4)
    assert _same(got_st, st) and _p_close(got_pv, pv)
    assert _same(stats.dwtest(rows[0]), dw[:1])                    # a 1-D input is one row
    recs = [(f"k{i}", s[i, :n]) for i, n in enumerate([100, 64, 100])]
    out = list(arima_diagnostics_partition(iter(recs), 2, 1, 2, 5))
    assert [r[0] for r in out] == ["k0", "k1", "k2"]
    for (key, coef, dw1, st1, pv1, acf1), (_, v) in zip(out, recs):
        one = ARIMA.fit_models(2, 1, 2, v[None, :])
        d1 = one.diagnostics(v[None, :], 5)
        assert _same(coef, one.coefficients[0]) and _same([dw1, st1, pv1], [d1.dw[0], d1.lb_stat[0], d1.lb_pvalue[0]])
        assert _same(acf1, d1.acf[0]), key


# ---- 8. the JNI shim forwards to the same ABI calls ----------------------------------------------------------------------
def test_jni_shim_diagnostics_match_direct_abi(engine):
    fn, env = jni_diag()
    h = fn("create")(env, None, 0)
    assert h != 0
    try:
        rng = np.random.default_rng(12)
        N, T, max_lag = 8, 120, 10
        s = np.ascontiguousarray(np.cumsum(rng.standard_normal((N, T)), axis=1))
        coef = rng.uniform(-0.3, 0.3, (N, 5))
        outs = [np.full((N, max_lag), SENT)] + [np.full(N, SENT) for _ in range(3)]
        rc = fn("diagnosticsBatch")(env, None, h, s.ctypes.data, N, T, max_lag, *[o.ctypes.data for o in outs])
        assert rc == 0, fn("lastError")(env, None, h)
        exp = engine.diagnostics(s, max_lag)
        assert all(_same(o, exp[k]) for o, k in zip(outs, L.Engine.DIAG_OUTPUTS))
        outs = [np.full((N, max_lag), SENT)] + [np.full(N, SENT) for _ in range(3)]
        rc = fn("residualDiagnosticsBatch")(env, None, h, s.ctypes.data, N, T, 2, 1, 2, 1, coef.ctypes.data, max_lag,
                                            outs[0].ctypes.data, None, outs[2].ctypes.data, outs[3].ctypes.data)
        assert rc == 0, fn("lastError")(env, None, h)
        exp = engine.residual_diagnostics(s, 2, 1, 2, True, coef, max_lag)
        assert _same(outs[0], exp["acf"]) and _same(outs[2], exp["lb_stat"]) and _same(outs[3], exp["lb_pvalue"])
        assert np.all(outs[1] == SENT)                             # a null output is not written
    finally:
        assert fn("destroy")(env, None, h) == 0
