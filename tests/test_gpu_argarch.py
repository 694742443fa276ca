"""ARGARCH, ARModel's pair and the GARCH / ARGARCH samples on the device against the pure-Python restatement
(tests/argarch_ref.py): the fused fit against the committed goldens (bit for bit, NaNs in the same places, host and device
entry points), short rows, tile edges, the fused fit against the unfused chain of existing entry points (results and
round counters), the pairs and samples (host and strided device forms) and the argument rules. Every comparison is
bit-exact."""
import ctypes

import numpy as np
import pytest

import argarch_ref as R
from conftest import load_case

pytestmark = pytest.mark.gpu

SENT = -7.25
FIT_KEYS = ("status", "n_eval", "n_grad", "coef", "obj")


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        bad = ~((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b)))
    else:
        bad = a != b
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist(), a[bad][:5], b[bad][:5])


def _same_fit(r, want, what=""):
    got = dict(r, obj=r["ll"])
    for k in FIT_KEYS:
        _same(got[k], want[k], f"{what} {k}")


# ---- the fit against the goldens --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FIXTURES)
def test_fit_parity_host(engine, name):
    meta, arr = load_case(name)
    _same_fit(engine.argarch_fit_batch(arr["series"]), arr, name)
    st = engine.model_fit_stats()
    assert st["n_series"] == meta["N"]
    assert st["max_wave_passes"] <= st["wave_passes"] <= st["lane_passes"] <= 64 * st["wave_passes"]


@pytest.mark.parametrize("name", R.FIXTURES)
def test_fit_parity_device_strided_with_guards(engine, name):
    import torch
    meta, arr = load_case(name)
    N, T = meta["N"], meta["T"]
    ld, G = T + 3, 8                                          # G sentinel rows before and after every output
    dev = f"cuda:{engine.device}"
    rows = torch.full((N, ld), SENT, dtype=torch.float64, device=dev)
    rows[:, :T] = torch.from_numpy(arr["series"]).to(dev)
    coef = torch.full((G + N + G, 5), SENT, dtype=torch.float64, device=dev)
    ll = torch.full((G + N + G,), SENT, dtype=torch.float64, device=dev)
    ints = [torch.full((G + N + G,), -77, dtype=torch.int32, device=dev) for _ in range(3)]
    engine.argarch_fit_batch_device(rows.data_ptr(), N, T, ld, coef[G:].data_ptr(), ll[G:].data_ptr(),
                                    ints[0][G:].data_ptr(), ints[1][G:].data_ptr(), ints[2][G:].data_ptr())
    got = dict(coef=coef[G:G + N].cpu().numpy(), ll=ll[G:G + N].cpu().numpy(),
               **{k: t[G:G + N].cpu().numpy() for k, t in zip(("status", "n_eval", "n_grad"), ints)})
    _same_fit(got, arr, name)
    for t in ints:
        assert bool((t[:G] == -77).all()) and bool((t[G + N:] == -77).all())
    for t in (coef, ll):
        assert bool((t[:G] == SENT).all()) and bool((t[G + N:] == SENT).all())
    assert bool((rows[:, T:] == SENT).all())
    _same(rows[:, :T].cpu().numpy(), arr["series"], "rows untouched")
    # the counters are optional
    st2 = torch.full((N,), -77, dtype=torch.int32, device=dev)
    engine.argarch_fit_batch_device(rows.data_ptr(), N, T, ld, coef[G:].data_ptr(), ll[G:].data_ptr(), st2.data_ptr())
    _same(st2.cpu().numpy(), arr["status"], "status without counters")


# ---- short rows and tile edges: the restatement computed here ----------------------------------------------------------
_FITS = {}


def _fit_reference(N, T):
    """argarch_rows(N, T, 40 + T) and the restatement's fits of them (once per shape)."""
    if (N, T) not in _FITS:
        rows = R.argarch_rows(N, T, 40 + T) if T > 13 else _short_rows(N, T)
        _FITS[(N, T)] = (rows, R.fit_batch(rows))
    return _FITS[(N, T)]


def _short_rows(N, T):
    rows = np.random.default_rng(40 + T).standard_normal((N, T))
    rows[5] = 0.0
    rows[6] = 3.25
    return rows


@pytest.mark.parametrize("T", (1, 2, 3, 4, 5))
def test_short_series(engine, T):
    rows, want = _fit_reference(16, T)
    if T == 1:
        assert np.all(want["status"] == R.ST_NO_DATA)
    elif T == 2:
        assert np.all(want["status"] == R.ST_NOT_ENOUGH_DATA)
    else:
        assert want["status"][5] == R.ST_SINGULAR            # the zero row (the constant row's QR can round off zero)
        assert set(want["status"].tolist()) <= {R.ST_OK, R.ST_SINGULAR, R.ST_MAX_EVAL}
    if T <= 2:
        assert np.all(np.isnan(want["coef"])) and np.all(np.isnan(want["obj"]))
        assert np.all(want["n_eval"] == 0) and np.all(want["n_grad"] == 0)
    _same_fit(engine.argarch_fit_batch(rows), want, f"T={T}")


def test_short_series_mix():
    # from T = 3 on the reference gives a mix of OK, _SINGULAR and _MAX_EVAL over the three short shapes
    seen = set()
    for T in (3, 4, 5):
        seen |= set(_fit_reference(16, T)[1]["status"].tolist())
    assert seen == {R.ST_OK, R.ST_SINGULAR, R.ST_MAX_EVAL}


@pytest.mark.parametrize("T", (32, 33, 64, 65))
def test_tile_edges(engine, T):
    # the carried raw value and the carried residual cross a tile boundary at t = 32 (and 64)
    rows, want = _fit_reference(16, T)
    assert (want["status"] == 0).sum() >= 8
    _same_fit(engine.argarch_fit_batch(rows), want, f"T={T}")


# ---- fused equals unfused ----------------------------------------------------------------------------------------------
def test_fused_equals_unfused_chain(engine):
    meta, arr = load_case("argarch/argarch_T97")
    rows = arr["series"]
    N = meta["N"]
    assert N == 130
    fused = engine.argarch_fit_batch(rows)
    ar = engine.fit_batch(rows, 1, 0, 0, True)
    ok = ar["status"] == 0
    _same(ar["status"], arr["ar_status"], "AR status")
    good = fused["status"] == 0
    _same(fused["coef"][good][:, :2], ar["coef"][good], "(c, phi)")
    # the rows whose AR stage failed have no residuals: the chain runs on the others
    res = engine.ar_remove_effects(rows[ok], 1, ar["coef"][ok])
    _same(res, np.array([R.ar_remove(r, c[0], [c[1]]) for r, c in zip(rows[ok].tolist(), ar["coef"][ok].tolist())]),
          "residuals")
    g = engine.garch_fit_batch(res)
    _same(fused["status"][ok], g["status"], "status")
    _same(fused["n_eval"][ok], g["n_eval"], "n_eval")
    _same(fused["n_grad"][ok], g["n_grad"], "n_grad")
    _same(fused["ll"][ok], g["ll"], "ll")
    _same(fused["coef"][ok][:, 2:], g["coef"], "(omega, alpha, beta)")
    assert np.all(fused["n_eval"][~ok] == 0) and np.all(fused["n_grad"][~ok] == 0)
    assert np.all(np.isnan(fused["coef"][~ok])) and np.all(np.isnan(fused["ll"][~ok]))


def test_fused_round_counters_equal_garch_on_residuals(engine):
    # the trajectories are bit-identical, so the fused fit runs exactly the rounds of a GARCH fit of the residual rows:
    # wave by wave, hence at the same N and row order. A row whose AR stage fails has no residuals, so the two such rows
    # of the fixture are replaced by copies of row 0 in the input of both fits
    meta, arr = load_case("argarch/argarch_T97")
    rows = arr["series"].copy()
    bad = arr["ar_status"] != 0
    rows[bad] = rows[0]
    N = rows.shape[0]
    assert N == 130
    fused = engine.argarch_fit_batch(rows)
    s_fused = engine.model_fit_stats()
    res = engine.ar_remove_effects(rows, 1, engine.fit_batch(rows, 1, 0, 0, True)["coef"])
    g = engine.garch_fit_batch(res)
    s_garch = engine.model_fit_stats()
    _same(fused["n_eval"], g["n_eval"], "n_eval")
    assert s_fused == s_garch, (s_fused, s_garch)
    assert s_fused["n_series"] == 130 and s_fused["lane_passes"] > 0


# ---- pairs and samples -------------------------------------------------------------------------------------------------
PAIR_NS = (1, 65, 130)


@pytest.mark.parametrize("T", (1, 2, 33, 97))
def test_pairs_and_samples_host(engine, T):
    ref = R.pair_reference(T)
    for N in PAIR_NS:
        rows, g = ref["rows"][:N], ref["g"][:N]
        _same(engine.argarch_remove_effects(rows, g), ref["argarch_remove"][:N], f"argarch remove N={N}")
        _same(engine.argarch_add_effects(rows, g), ref["argarch_add"][:N], f"argarch add N={N}")
        gs, as_ = engine.garch_sample(rows, g[:, 2:]), engine.argarch_sample(rows, g)
        _same(gs, ref["garch_sample"][:N], f"garch sample N={N}")
        _same(as_, ref["argarch_sample"][:N], f"argarch sample N={N}")
        assert np.all(gs[:, 0].view(np.int64) == 0) and np.all(as_[:, 0].view(np.int64) == 0)     # +0.0, never assigned
        for p in R.AR_ORDERS:                                  # includes T < p: only the lags that exist
            a = ref["ar"][p][:N]
            _same(engine.ar_remove_effects(rows, p, a), ref[f"ar_remove_{p}"][:N], f"ar remove p={p} N={N}")
            _same(engine.ar_add_effects(rows, p, a), ref[f"ar_add_{p}"][:N], f"ar add / sample p={p} N={N}")


@pytest.mark.parametrize("T", (1, 2, 33, 97))
def test_pairs_and_samples_device_strided(engine, T):
    import torch
    ref = R.pair_reference(T)
    dev = f"cuda:{engine.device}"
    ld, ldo = T + 3, T + 5
    for N in PAIR_NS:
        d_in = torch.full((N, ld), SENT, dtype=torch.float64, device=dev)
        d_in[:, :T] = torch.from_numpy(ref["rows"][:N]).to(dev)
        d_g = torch.from_numpy(np.ascontiguousarray(ref["g"][:N])).to(dev)
        d_g3 = torch.from_numpy(np.ascontiguousarray(ref["g"][:N, 2:])).to(dev)

        def run(call, want, what):
            d_out = torch.full((N, ldo), SENT, dtype=torch.float64, device=dev)
            call(d_out)
            _same(d_out[:, :T].cpu().numpy(), want[:N], f"{what} N={N}")
            assert bool((d_out[:, T:] == SENT).all()), what

        for d in ("remove", "add"):
            run(lambda o: engine.model_effects_device("argarch", d, d_in.data_ptr(), N, T, ld, d_g.data_ptr(),
                                                      o.data_ptr(), ldo), ref[f"argarch_{d}"], f"argarch {d}")
        run(lambda o: engine.model_sample_device("garch", d_in.data_ptr(), N, T, ld, d_g3.data_ptr(), o.data_ptr(), ldo),
            ref["garch_sample"], "garch sample")
        run(lambda o: engine.model_sample_device("argarch", d_in.data_ptr(), N, T, ld, d_g.data_ptr(), o.data_ptr(), ldo),
            ref["argarch_sample"], "argarch sample")
        for p in R.AR_ORDERS:
            d_a = torch.from_numpy(np.ascontiguousarray(ref["ar"][p][:N])).to(dev)
            for d in ("remove", "add"):
                run(lambda o: engine.ar_effects_device(d, d_in.data_ptr(), N, T, ld, p, d_a.data_ptr(), o.data_ptr(), ldo),
                    ref[f"ar_{d}_{p}"], f"ar {d} p={p}")
        assert bool((d_in[:, T:] == SENT).all())


def test_argarch_round_trip(engine):
    # GARCHSuite "standardize and filter" through the device: sample, remove, add
    model = (40.0, .4, .2, .3, .4)
    z = np.random.default_rng(5).standard_normal(2000)
    ts = engine.argarch_sample(z, model)
    back = engine.argarch_add_effects(engine.argarch_remove_effects(ts, model), model)
    assert ts[0, 0] == 0.0 and np.max(np.abs(back - ts)) < 1e-3


# ---- argument rules ----------------------------------------------------------------------------------------------------
def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def test_argument_rules_host(engine):
    L, h = engine.L, engine.h
    rows = np.ones((4, 6))
    c3, c5, obj = np.full((4, 3), SENT), np.full((4, 5), SENT), np.full(4, SENT)
    c21 = np.full((4, 21), SENT)
    st = np.full(4, -77, np.int32)
    out = np.full((4, 6), SENT)
    fit = L.arima_argarch_fit_batch
    # T == 0: the fit refuses; N == 0: nothing to do
    assert fit(h, _dp(rows), 4, 0, _dp(c5), _dp(obj), _ip(st), None, None) == -1
    assert fit(h, _dp(rows), 0, 6, _dp(c5), _dp(obj), _ip(st), None, None) == 0
    # outputs of a fit may not meet the rows or one another
    assert fit(h, _dp(rows), 4, 6, _dp(rows), _dp(obj), _ip(st), None, None) == -1
    assert fit(h, _dp(rows), 4, 6, _dp(c5), _dp(c5[3:]), _ip(st), None, None) == -1
    assert fit(h, _dp(rows), 4, 6, _dp(c5), _dp(obj), _ip(st), _ip(st), None) == -1
    for fn, par in ((L.arima_argarch_remove_effects_batch, c5), (L.arima_argarch_add_effects_batch, c5),
                    (L.arima_garch_sample_batch, c3), (L.arima_argarch_sample_batch, c5)):
        assert fn(h, _dp(rows), 0, 6, _dp(par), _dp(out)) == 0
        assert fn(h, _dp(rows), 4, 0, _dp(par), _dp(out)) == 0
        # no in-place form, no output over the parameters
        assert fn(h, _dp(rows), 4, 6, _dp(par), _dp(rows)) == -1
        big = np.ones(4 * 6 + 20)
        assert fn(h, _dp(rows), 4, 6, _dp(big), _dp(big[2:])) == -1
    for fn in (L.arima_ar_remove_effects_batch, L.arima_ar_add_effects_batch):
        assert fn(h, _dp(rows), 0, 6, 2, _dp(c3), _dp(out)) == 0
        assert fn(h, _dp(rows), 4, 0, 2, _dp(c3), _dp(out)) == 0
        assert fn(h, _dp(rows), 4, 6, 2, _dp(c3), _dp(rows)) == -1
        big = np.ones(4 * 6 + 20)
        assert fn(h, _dp(rows), 4, 6, 2, _dp(big), _dp(big[2:])) == -1
        # p out of range: below 1 is invalid, above the library's order limit unsupported (also with nothing to do)
        assert fn(h, _dp(rows), 4, 6, 0, _dp(c3), _dp(out)) == -1
        assert fn(h, _dp(rows), 4, 6, -1, _dp(c3), _dp(out)) == -1
        assert fn(h, _dp(rows), 4, 6, 21, _dp(np.full((4, 22), .1)), _dp(out)) == -2
        assert fn(h, _dp(rows), 0, 6, 21, _dp(c21), _dp(out)) == -2
        assert fn(h, _dp(rows), 4, 6, 20, _dp(np.full((4, 21), .01)), _dp(np.empty((4, 6)))) == 0
    assert np.all(out == SENT) and np.all(c3 == SENT) and np.all(c5 == SENT) and np.all(obj == SENT)
    assert np.all(st == -77) and np.all(rows == 1.0)


def test_argument_rules_device(engine):
    import torch
    dev = f"cuda:{engine.device}"
    L, h = engine.L, engine.h
    N, T = 5, 20
    rows = torch.ones((N, 24), dtype=torch.float64, device=dev)
    out = torch.full((N, 24), SENT, dtype=torch.float64, device=dev)
    par = torch.full((N, 5), .2, dtype=torch.float64, device=dev)
    obj = torch.full((N,), SENT, dtype=torch.float64, device=dev)
    st = torch.full((N,), -77, dtype=torch.int32, device=dev)
    fit = L.arima_argarch_fit_batch_device
    assert fit(h, rows.data_ptr(), N, T, T - 1, par.data_ptr(), obj.data_ptr(), st.data_ptr(), None, None, None) == -1
    assert fit(h, rows.data_ptr(), N, 0, 24, par.data_ptr(), obj.data_ptr(), st.data_ptr(), None, None, None) == -1
    assert fit(h, rows.data_ptr(), N, T, 24, rows.data_ptr() + 8, obj.data_ptr(), st.data_ptr(), None, None, None) == -1
    assert fit(h, rows.data_ptr(), 0, T, 24, par.data_ptr(), obj.data_ptr(), st.data_ptr(), None, None, None) == 0
    calls = [(getattr(L, f"arima_{m}_batch_device"), ()) for m in
             ("argarch_remove_effects", "argarch_add_effects", "garch_sample", "argarch_sample")]
    calls += [(getattr(L, f"arima_ar_{d}_effects_batch_device"), (3,)) for d in ("remove", "add")]
    for fx, order in calls:
        args = lambda n, t, ld, o, ldo: (h, rows.data_ptr(), n, t, ld) + order + (par.data_ptr(), o, ldo, None)
        assert fx(*args(N, T, T - 1, out.data_ptr(), 24)) == -1
        assert fx(*args(N, T, 24, out.data_ptr(), T - 1)) == -1
        assert fx(*args(N, T, 24, rows.data_ptr(), 24)) == -1
        assert fx(*args(N, T, 24, rows.data_ptr() + 8 * T, 24)) == -1
        assert fx(*args(N, T, 24, par.data_ptr(), 24)) == -1
        assert fx(*args(0, T, 24, out.data_ptr(), 24)) == 0
        assert fx(*args(N, 0, 24, out.data_ptr(), 24)) == 0
    for d in ("remove", "add"):
        fx = getattr(L, f"arima_ar_{d}_effects_batch_device")
        assert fx(h, rows.data_ptr(), N, T, 24, 0, par.data_ptr(), out.data_ptr(), 24, None) == -1
        assert fx(h, rows.data_ptr(), N, T, 24, 21, par.data_ptr(), out.data_ptr(), 24, None) == -2
    engine.synchronize()
    assert bool((out == SENT).all()) and bool((obj == SENT).all()) and bool((st == -77).all())
    assert bool((rows == 1.0).all()) and bool((par == .2).all())
