"""ARIMAModel.removeTimeDependentEffects / addTimeDependentEffects (ARIMA.scala:629-667) on the GPU against the CPU
restatement (oracle.remove_time_dependent_effects / add_time_dependent_effects, pinned to ARIMASuite.scala:99-112 by
tests/test_oracle_kats.py), row by row and bit for bit: the tiled kernel (p, q <= 5, d <= 8), the runtime-order kernel,
tile edges and strides through the device entry points, in-place calls, refused overlaps, short series, special
values, the round trip, residuals of fitted models through the Python mirror, and the JNI shim."""
import numpy as np
import pytest

import oracle as O
import sparkts_amd._lib as L
from test_effects import jni_effects

pytestmark = pytest.mark.gpu

ARIMA_E_INVALID_ARG = -1
REMOVE, ADD = "remove", "add"
ORACLE = {REMOVE: O.remove_time_dependent_effects, ADD: O.add_time_dependent_effects}


def _same(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.array_equal(a.view(np.int64) if a.size else a, b.view(np.int64) if b.size else b) or \
        np.array_equal(a, b, equal_nan=True)


def _same_signed(a, b):
    """_same, and the sign of every zero agrees too (NaN payloads and signs are not compared)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    num = ~np.isnan(b)
    return _same(a, b) and np.array_equal(np.signbit(a[num]), np.signbit(b[num]))


def _host(engine, which):
    return engine.remove_effects if which == REMOVE else engine.add_effects


def _dev(engine, which):
    return engine.remove_effects_device if which == REMOVE else engine.add_effects_device


def _dev_abi(engine, which):
    return getattr(engine.L, f"arima_{which}_effects_batch_device")


def _oracle(which, rows, p, d, q, I, coef):
    return np.stack([ORACLE[which](rows[i], p, d, q, I, coef[i]) for i in range(rows.shape[0])])


# ---- 1. both directions at the orders of test_forecast_bit_exact, and three runtime-order cases -------------------
TILED = [(1, 0, 1, 1), (2, 1, 2, 1), (2, 1, 2, 0), (0, 1, 3, 1), (3, 3, 1, 0), (5, 1, 5, 1), (0, 2, 0, 1), (1, 8, 1, 1)]
RUNTIME_ORDER = [(7, 1, 2, 1), (2, 0, 20, 0), (1, 9, 1, 1)]


@pytest.mark.parametrize("which", [REMOVE, ADD])
@pytest.mark.parametrize("pdqi", TILED + RUNTIME_ORDER)
def test_effects_bit_exact(engine, pdqi, which):
    p, d, q, I = pdqi
    rng = np.random.default_rng(1000 + 97 * p + 13 * d + q + I)
    N, T = 96, 211
    s = rng.standard_normal((N, T)).cumsum(axis=1) * 3.0 + 5.0
    coef = rng.uniform(-0.6, 0.6, (N, p + q + I))
    out = _host(engine, which)(s, p, d, q, I, coef)
    exp = _oracle(which, s, p, d, q, I, coef)
    assert out.shape == (N, T)
    assert _same(out, exp), (pdqi, which, np.nanmax(np.abs(out - exp)))


# ---- 2. tile edges through the device entry points: [64 series x 32 steps] tiles, strided rows, in place ----------
@pytest.mark.parametrize("which", [REMOVE, ADD])
@pytest.mark.parametrize("N", [1, 64, 65])
@pytest.mark.parametrize("T", [1, 31, 32, 33, 65])
def test_effects_tile_edges(engine, T, N, which):
    import torch
    ld, ldo = T + 8, T + 13
    for p, d, q, I in [(2, 1, 2, 1), (7, 1, 2, 1)]:              # the tiled and the runtime-order kernel
        rng = np.random.default_rng(31 * T + N + p)
        s = rng.standard_normal((N, T)).cumsum(axis=1) + 2.0
        coef = rng.uniform(-0.5, 0.5, (N, p + q + I))
        exp = _oracle(which, s, p, d, q, I, coef)
        sd = torch.full((N, ld), 3.25, dtype=torch.float64, device="cuda")
        sd[:, :T] = torch.from_numpy(s).cuda()
        cd = torch.from_numpy(coef).cuda().contiguous()
        od = torch.full((N, ldo), -7.0, dtype=torch.float64, device="cuda")
        _dev(engine, which)(sd.data_ptr(), N, T, ld, p, d, q, I, cd.data_ptr(), od.data_ptr(), ldo)
        torch.cuda.synchronize()
        o = od.cpu().numpy()
        assert _same(o[:, :T], exp), (p, T, N, which)
        assert np.all(o[:, T:] == -7.0)                          # nothing written beyond column T
        # the same call in place (d_out == d_in, equal strides): the same bits, the padding untouched
        _dev(engine, which)(sd.data_ptr(), N, T, ld, p, d, q, I, cd.data_ptr(), sd.data_ptr(), ld)
        torch.cuda.synchronize()
        o = sd.cpu().numpy()
        assert _same(o[:, :T], exp), ("in place", p, T, N, which)
        assert np.all(o[:, T:] == 3.25)


@pytest.mark.parametrize("which", [REMOVE, ADD])
def test_effects_refuse_overlapping_output(engine, which):
    # refused by the argument check, before any launch: nothing is written
    import torch
    N, T, ld = 4, 33, 41
    buf = torch.full((2 * N * ld,), -7.0, dtype=torch.float64, device="cuda")
    cd = torch.zeros((N, 5), dtype=torch.float64, device="cuda")
    base = buf.data_ptr()
    abi = _dev_abi(engine, which)
    for out_ptr, ldo in [(base + 5 * 8, ld),                     # shifted by five elements
                         (base, ld + 1),                         # the same start, another stride
                         (base + (N - 1) * ld * 8, ld)]:         # its first row is the input's last
        assert abi(engine.h, base, N, T, ld, 2, 1, 2, 1, cd.data_ptr(), out_ptr, ldo, None) == ARIMA_E_INVALID_ARG
    # the coefficients inside the output range
    assert abi(engine.h, base, N, T, ld, 2, 1, 2, 1, base + N * ld * 8 + 16, base + N * ld * 8, ld,
               None) == ARIMA_E_INVALID_ARG
    for bad_ld, bad_ldo in [(T - 1, ld), (ld, T - 1)]:
        assert abi(engine.h, base, N, T, bad_ld, 2, 1, 2, 1, cd.data_ptr(), base + N * ld * 8, bad_ldo,
                   None) == ARIMA_E_INVALID_ARG
    engine.synchronize()
    assert bool(torch.all(buf == -7.0))
    # N == 0 and T == 0 are fine and write nothing
    assert abi(engine.h, base, 0, T, ld, 2, 1, 2, 1, cd.data_ptr(), base + N * ld * 8, ld, None) == 0
    assert abi(engine.h, base, N, 0, ld, 2, 0, 2, 1, cd.data_ptr(), base + N * ld * 8, ld, None) == 0
    engine.synchronize()
    assert bool(torch.all(buf == -7.0))


# ---- 3. series barely longer than d and shorter than max(p, q) ----------------------------------------------------
@pytest.mark.parametrize("which", [REMOVE, ADD])
@pytest.mark.parametrize("T", [1, 2, 3, 6])
def test_effects_short_series(engine, T, which):
    rng = np.random.default_rng(T)
    for p, d, q, I in [(2, 2, 3, 1), (5, 1, 5, 0), (1, 2, 1, 1)]:
        s = rng.standard_normal((8, T))
        coef = rng.uniform(-0.5, 0.5, (8, p + q + I))
        if T < d:
            out = np.full((8, T), -7.0)
            dp = L._dp
            rc = getattr(engine.L, f"arima_{which}_effects_batch")(engine.h, s.ctypes.data_as(dp), 8, T, p, d, q, I,
                                                                   coef.ctypes.data_as(dp), out.ctypes.data_as(dp))
            assert rc == ARIMA_E_INVALID_ARG and np.all(out == -7.0)
            continue
        assert _same(_host(engine, which)(s, p, d, q, I, coef), _oracle(which, s, p, d, q, I, coef)), (T, p, d, q, I)


# ---- 4. special values --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [REMOVE, ADD])
@pytest.mark.parametrize("pdqi", [(2, 1, 2, 0), (1, 0, 1, 1)])
def test_effects_special_values(engine, pdqi, which):
    p, d, q, I = pdqi
    k = p + q + I
    rng = np.random.default_rng(5 + p)
    N, T = 70, 75
    s = rng.standard_normal((N, T))
    coef = rng.uniform(-0.6, 0.6, (N, k))
    clean = _host(engine, which)(s, p, d, q, I, coef)
    s2 = s.copy()
    s2[3, 40] = np.nan                                           # a NaN inside one series
    s2[9, ::2] = -0.0                                            # negative zeros in the input
    s2[10, :] = -0.0
    s2[66, 0] = -0.0
    out = _host(engine, which)(s2, p, d, q, I, coef)
    assert _same_signed(out, _oracle(which, s2, p, d, q, I, coef))
    touched = np.zeros(N, bool)
    touched[[3, 9, 10, 66]] = True
    assert _same(out[~touched], clean[~touched])                 # every other row is unchanged
    assert np.all(np.isnan(out[3, 40:])) and _same(out[3, :40], clean[3, :40])
    # coefficient rows holding NaN, +inf and -0.0 (without an intercept coef[0] still multiplies the 0.0 intercept
    # flag: NaN and inf poison the row, as in the reference)
    c2 = coef.copy()
    c2[0, 0] = np.nan
    c2[1, 0] = np.inf
    c2[2, 0] = -0.0
    c2[4, :] = -0.0
    c2[5, k - 1] = np.nan
    c2[6, k - 1] = np.inf
    c2[65, 0] = -0.5                                             # 0 * negative = -0.0 without an intercept
    for rows in (s, s2):
        out = _host(engine, which)(rows, p, d, q, I, c2)
        assert _same_signed(out, _oracle(which, rows, p, d, q, I, c2)), (pdqi, which)
    assert np.all(np.isnan(out[0]))
    if not I:
        assert np.all(np.isnan(out[1]))                          # 0.0 * inf


# ---- 5. the round trip of ARIMASuite.scala:99-112 -----------------------------------------------------------------
def test_effects_round_trip(engine):
    p, d, q, I = 1, 1, 2, 1
    coef = np.array([8.3, 0.1, 0.2, 0.3])
    N, T = 64, 100
    e = np.random.default_rng(10).standard_normal((N, T))
    cn = np.tile(coef, (N, 1))
    added = engine.add_effects(e, p, d, q, I, coef)
    back = engine.remove_effects(added, p, d, q, I, coef)
    exp_added = _oracle(ADD, e, p, d, q, I, cn)
    assert _same(added, exp_added)
    assert _same(back, _oracle(REMOVE, exp_added, p, d, q, I, cn))
    assert np.all(np.abs(back - e) < 1e-4)                       # the reference suite's own bound


# ---- 6. residuals after a fit, through the Python mirror ----------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(engine):
    import torch
    from sparkts_amd.models import ARIMA
    N, T = 256, 256
    buf = torch.empty((N, T), dtype=torch.float64, device="cuda")
    engine.sample_device(buf.data_ptr(), N, T, T, 2, 1, 2, 1, [8.2, 0.2, 0.5, 0.3, 0.1], 0.05, 20261015)
    s = np.concatenate([buf.cpu().numpy(), np.full((1, T), np.nan)])     # and one series no fit can handle
    return s, ARIMA.fit_models(2, 1, 2, s)


def test_residuals_of_fitted_models(engine, fitted):
    from sparkts_amd.models import ARIMA
    s, res = fitted
    ok = res.status == L.ST_OK
    assert ok[:256].mean() > 0.9 and not ok[256]
    r = res.residuals(s)
    assert r.shape == s.shape
    exp = _oracle(REMOVE, s[ok], 2, 1, 2, 1, res.coefficients[ok])
    assert _same(r[ok], exp)
    assert np.all(np.isnan(r[~ok]))
    assert ok[0]
    m = res.model(0)
    assert _same(m.remove_time_dependent_effects(s[0]), r[0])
    dest = np.zeros(s.shape[1])
    assert m.remove_time_dependent_effects(s[0], dest) is dest and _same(dest, r[0])
    noise = r[0].copy()
    assert m.add_time_dependent_effects(noise, noise) is noise           # sample's addTimeDependentEffects(vec, vec)
    assert _same(noise, O.add_time_dependent_effects(r[0], 2, 1, 2, 1, m.coefficients))
    assert isinstance(m, ARIMA.ARIMAModel)


def test_residuals_partition_keeps_input_order(engine, fitted):
    from sparkts_amd.timeseriesrdd import arima_residuals_partition
    s, _ = fitted
    lens = [64, 100, 100, 64, 100, 64, 64]
    recs = [(f"k{i}", s[i, :n]) for i, n in enumerate(lens)]
    out = list(arima_residuals_partition(iter(recs), 2, 1, 2))
    assert [k for k, _, _ in out] == [k for k, _ in recs]
    for (key, coef, resid), (_, v) in zip(out, recs):
        one = engine.fit_batch(v, 2, 1, 2, True)
        assert _same(coef, one["coef"][0]), key
        assert resid.shape == v.shape
        if one["status"][0] == L.ST_OK:
            assert _same(resid, O.remove_time_dependent_effects(v, 2, 1, 2, 1, coef)), key
        else:
            assert np.all(np.isnan(resid)), key


# ---- 7. the JNI shim forwards to the same ABI calls ---------------------------------------------------------------
def test_jni_shim_effects_match_direct_abi(engine):
    fn, env = jni_effects()
    h = fn("create")(env, None, 0)
    assert h != 0
    try:
        rng = np.random.default_rng(12)
        N, T = 300, 256
        s = np.ascontiguousarray(np.cumsum(rng.standard_normal((N, T)), axis=1))
        coef = rng.uniform(-0.6, 0.6, (N, 5))
        for name, direct in (("removeEffectsBatch", engine.remove_effects), ("addEffectsBatch", engine.add_effects)):
            out = np.full((N, T), -7.0)
            rc = fn(name)(env, None, h, s.ctypes.data, N, T, 2, 1, 2, 1, coef.ctypes.data, out.ctypes.data)
            assert rc == 0, fn("lastError")(env, None, h)
            assert _same(out, direct(s, 2, 1, 2, True, coef)), name
    finally:
        assert fn("destroy")(env, None, h) == 0
