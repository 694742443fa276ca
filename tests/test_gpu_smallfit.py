"""EWMA and GARCH(1,1) on the device against the pure-Python restatement (tests/smallfit_ref.py): the fits against the
committed goldens (bit for bit, NaNs in the same places, host and device entry points), the building blocks and the
TimeSeriesModel pairs against the restatement computed here (tile width 32 and its neighbours, wave size 64 and its
neighbours, strided rows, special parameters), the argument rules, the Python layer and the JNI natives."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import smallfit_ref as R
from conftest import ROOT, load_case

pytestmark = pytest.mark.gpu

SENT = -7.25
NS = (1, 63, 64, 65, 130)
TS = (1, 2, 31, 32, 33, 65, 100)


def _same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        bad = ~((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b)))
    else:
        bad = a != b
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist(), a[bad][:5], b[bad][:5])


# ---- fits against the goldens ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FIXTURES)
def test_fit_parity_host(engine, name):
    meta, arr = load_case(name)
    if meta["model"] == "ewma":
        r = engine.ewma_fit_batch(arr["series"])
        coef, obj = r["smoothing"][:, None], r["sse"]
    else:
        r = engine.garch_fit_batch(arr["series"])
        coef, obj = r["coef"], r["ll"]
    _same(r["status"], arr["status"], "status")
    _same(r["n_eval"], arr["n_eval"], "n_eval")
    _same(r["n_grad"], arr["n_grad"], "n_grad")
    _same(coef, arr["coef"], "coef")
    _same(obj, arr["obj"], "obj")
    st = engine.model_fit_stats()
    # a pass per posted point: every gradient and every evaluation but the one at the top of an iteration (which reuses
    # the value that came with the gradient); a fit that returns normally has as many iterations as gradients
    ok = arr["status"] == 0
    assert st["n_series"] == 130
    assert int(arr["n_eval"][ok].sum()) <= st["lane_passes"] - int(arr["n_eval"][~ok].sum()) <= int(arr["n_eval"][ok].sum()) + 4
    assert st["max_wave_passes"] <= st["wave_passes"] <= st["lane_passes"] <= 64 * st["wave_passes"]


@pytest.mark.parametrize("name", R.FIXTURES)
def test_fit_parity_device_strided_with_guards(engine, name):
    import torch
    meta, arr = load_case(name)
    N, T, K = meta["N"], meta["T"], arr["coef"].shape[1]
    ld, G = T + 5, 8
    dev = f"cuda:{engine.device}"
    rows = torch.full((N, ld), SENT, dtype=torch.float64, device=dev)
    rows[:, :T] = torch.from_numpy(arr["series"]).to(dev)
    coef = torch.full((N * K + G,), SENT, dtype=torch.float64, device=dev)
    obj = torch.full((N + G,), SENT, dtype=torch.float64, device=dev)
    ints = [torch.full((N + G,), -77, dtype=torch.int32, device=dev) for _ in range(3)]
    fit = engine.ewma_fit_batch_device if meta["model"] == "ewma" else engine.garch_fit_batch_device
    fit(rows.data_ptr(), N, T, ld, coef.data_ptr(), obj.data_ptr(), ints[0].data_ptr(), ints[1].data_ptr(),
        ints[2].data_ptr())
    _same(coef[:N * K].cpu().numpy().reshape(N, K), arr["coef"], "coef")
    _same(obj[:N].cpu().numpy(), arr["obj"], "obj")
    for t, k in zip(ints, ("status", "n_eval", "n_grad")):
        _same(t[:N].cpu().numpy(), arr[k], k)
        assert bool((t[N:] == -77).all()), k
    assert bool((coef[N * K:] == SENT).all()) and bool((obj[N:] == SENT).all())
    assert bool((rows[:, T:] == SENT).all())
    # the counters are optional
    st2 = torch.full((N,), -77, dtype=torch.int32, device=dev)
    fit(rows.data_ptr(), N, T, ld, coef.data_ptr(), obj.data_ptr(), st2.data_ptr())
    _same(st2.cpu().numpy(), arr["status"], "status without counters")


# ---- building blocks and effects against the restatement ------------------------------------------------------------
def _params(N):
    rng = np.random.default_rng(99)
    sm = rng.uniform(0.05, 1.5, N)
    sm[0], sm[min(1, N - 1)] = -0.3, 1.7
    g = np.stack([rng.uniform(.05, .5, N), rng.uniform(.05, .4, N), rng.uniform(.05, .5, N)], axis=1)
    if N > 8:
        sm[2], sm[3] = np.nan, 0.0                           # NaN parameter; remove divides by zero
        g[4, 1:] = (.5, .5)                                  # alpha + beta = 1: prevH = omega / 0
        g[5, 0] = np.nan
        g[6, 1] = -.2
        g[7] = (.2, .3, .4)
    return sm, g


_REF = {}


def _reference(T):
    """The restatement over 130 rows of length T (computed once per T; smaller N take the first rows)."""
    if T not in _REF:
        rng = np.random.default_rng(1000 + T)
        rows = rng.standard_normal((130, T))
        rows[8] *= 1e160                                     # overflows to Inf in the squares
        if T > 2:
            rows[9, T // 2] = np.nan
        sm_a, g_a = _params(130)
        sm, g = sm_a.tolist(), g_a.tolist()                 # Python floats: IEEE results without numpy's warnings
        ref = dict(rows=rows, sm=sm_a, g=g_a,
                   sse=np.array([R.ewma_sse(r.tolist(), a) for r, a in zip(rows, sm)]),
                   egrad=np.array([R.ewma_gradient(r.tolist(), a) for r, a in zip(rows, sm)]),
                   ll=np.array([R.garch_loglik(r.tolist(), *c) for r, c in zip(rows, g)]),
                   ggrad=np.array([R.garch_gradient(r.tolist(), *c) for r, c in zip(rows, g)]),
                   ewma_remove=np.array([R.ewma_remove(r.tolist(), a) for r, a in zip(rows, sm)]),
                   ewma_add=np.array([R.ewma_add(r.tolist(), a) for r, a in zip(rows, sm)]),
                   garch_remove=np.array([R.garch_remove(r.tolist(), *c) for r, c in zip(rows, g)]),
                   garch_add=np.array([R.garch_add(r.tolist(), *c) for r, c in zip(rows, g)]))
        _REF[T] = ref
    return _REF[T]


@pytest.mark.parametrize("T", TS)
def test_building_blocks(engine, T):
    ref = _reference(T)
    for N in NS:
        rows, sm, g = ref["rows"][:N], ref["sm"][:N], ref["g"][:N]
        _same(engine.ewma_sse(rows, sm), ref["sse"][:N], f"sse N={N}")
        _same(engine.ewma_gradient(rows, sm), ref["egrad"][:N], f"ewma gradient N={N}")
        _same(engine.garch_loglik(rows, g), ref["ll"][:N], f"loglik N={N}")
        _same(engine.garch_gradient(rows, g), ref["ggrad"][:N], f"garch gradient N={N}")


@pytest.mark.parametrize("T", TS)
def test_effects_host_and_strided_device(engine, T):
    import torch
    ref = _reference(T)
    dev = f"cuda:{engine.device}"
    for N in NS:
        rows = ref["rows"][:N]
        for model, par in (("ewma", ref["sm"][:N]), ("garch", ref["g"][:N])):
            for direction in ("remove", "add"):
                want = ref[f"{model}_{direction}"][:N]
                got = getattr(engine, f"{model}_{direction}_effects")(rows, par)
                _same(got, want, f"{model} {direction} host N={N}")
        # device entry points: independent strides, sentinel padding
        ld, ldo = T + 3, T + 5
        d_in = torch.full((N, ld), SENT, dtype=torch.float64, device=dev)
        d_in[:, :T] = torch.from_numpy(rows).to(dev)
        for model, par in (("ewma", ref["sm"][:N]), ("garch", ref["g"][:N])):
            d_par = torch.from_numpy(np.ascontiguousarray(par)).to(dev)
            for direction in ("remove", "add"):
                d_out = torch.full((N, ldo), SENT, dtype=torch.float64, device=dev)
                engine.model_effects_device(model, direction, d_in.data_ptr(), N, T, ld, d_par.data_ptr(),
                                            d_out.data_ptr(), ldo)
                _same(d_out[:, :T].cpu().numpy(), ref[f"{model}_{direction}"][:N], f"{model} {direction} dev N={N}")
                assert bool((d_out[:, T:] == SENT).all())


def test_garch_round_trip(engine):
    # GARCHSuite "standardize and filter": add after remove returns the series
    rng = np.random.default_rng(5)
    ts = np.asarray(R.garch_add(rng.standard_normal(2000).tolist(), .2, .3, .4))
    back = engine.garch_add_effects(engine.garch_remove_effects(ts, (.2, .3, .4)), (.2, .3, .4))[0]
    assert np.max(np.abs(back - ts)) < 1e-3


# ---- argument rules ----------------------------------------------------------------------------------------------
def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def test_argument_rules_host(engine):
    L, h = engine.L, engine.h
    rows = np.ones((4, 6))
    c1, c3, obj = np.full(4, SENT), np.full((4, 3), SENT), np.full(4, SENT)
    st = np.full(4, -77, np.int32)
    # T == 0: fits and building blocks refuse
    assert L.arima_ewma_fit_batch(h, _dp(rows), 4, 0, _dp(c1), _dp(obj), _ip(st), None, None) == -1
    assert L.arima_garch_fit_batch(h, _dp(rows), 4, 0, _dp(c3), _dp(obj), _ip(st), None, None) == -1
    assert L.arima_ewma_sse_batch(h, _dp(rows), 4, 0, _dp(c1), _dp(obj)) == -1
    assert L.arima_garch_gradient_batch(h, _dp(rows), 4, 0, _dp(c3), _dp(np.empty((4, 3)))) == -1
    # N == 0: nothing to do
    assert L.arima_ewma_fit_batch(h, _dp(rows), 0, 6, _dp(c1), _dp(obj), _ip(st), None, None) == 0
    out = np.full((4, 6), SENT)
    for fn, par in ((L.arima_ewma_remove_effects_batch, c1), (L.arima_ewma_add_effects_batch, c1),
                    (L.arima_garch_remove_effects_batch, c3), (L.arima_garch_add_effects_batch, c3)):
        assert fn(h, _dp(rows), 0, 6, _dp(par), _dp(out)) == 0
        assert fn(h, _dp(rows), 4, 0, _dp(par), _dp(out)) == 0
        # no in-place form, no output over the parameters
        assert fn(h, _dp(rows), 4, 6, _dp(par), _dp(rows)) == -1
        big = np.ones(4 * 6 + 12)
        assert fn(h, _dp(rows), 4, 6, _dp(big), _dp(big[2:])) == -1
    # outputs of a fit may not meet the rows or one another
    assert L.arima_ewma_fit_batch(h, _dp(rows), 4, 6, _dp(rows), _dp(obj), _ip(st), None, None) == -1
    assert L.arima_ewma_fit_batch(h, _dp(rows), 4, 6, _dp(obj), _dp(obj), _ip(st), None, None) == -1
    assert L.arima_garch_fit_batch(h, _dp(rows), 4, 6, _dp(c3), _dp(c3[1:]), _ip(st), None, None) == -1
    assert L.arima_garch_fit_batch(h, _dp(rows), 4, 6, _dp(c3), _dp(obj), _ip(st), _ip(st), None) == -1
    assert np.all(out == SENT) and np.all(c1 == SENT) and np.all(c3 == SENT) and np.all(obj == SENT)
    assert np.all(st == -77) and np.all(rows == 1.0)


def test_argument_rules_device(engine):
    import torch
    dev = f"cuda:{engine.device}"
    L, h = engine.L, engine.h
    N, T = 5, 20
    rows = torch.ones((N, 24), dtype=torch.float64, device=dev)
    out = torch.full((N, 24), SENT, dtype=torch.float64, device=dev)
    par = torch.full((N, 3), .2, dtype=torch.float64, device=dev)
    obj = torch.full((N,), SENT, dtype=torch.float64, device=dev)
    st = torch.full((N,), -77, dtype=torch.int32, device=dev)
    for m in ("ewma", "garch"):
        fit = getattr(L, f"arima_{m}_fit_batch_device")
        assert fit(h, rows.data_ptr(), N, T, T - 1, par.data_ptr(), obj.data_ptr(), st.data_ptr(), None, None, None) == -1
        assert fit(h, rows.data_ptr(), N, 0, 24, par.data_ptr(), obj.data_ptr(), st.data_ptr(), None, None, None) == -1
        assert fit(h, rows.data_ptr(), N, T, 24, rows.data_ptr() + 8, obj.data_ptr(), st.data_ptr(), None, None,
                   None) == -1
        for d in ("remove", "add"):
            fx = getattr(L, f"arima_{m}_{d}_effects_batch_device")
            assert fx(h, rows.data_ptr(), N, T, T - 1, par.data_ptr(), out.data_ptr(), 24, None) == -1
            assert fx(h, rows.data_ptr(), N, T, 24, par.data_ptr(), out.data_ptr(), T - 1, None) == -1
            assert fx(h, rows.data_ptr(), N, T, 24, par.data_ptr(), rows.data_ptr(), 24, None) == -1
            assert fx(h, rows.data_ptr(), N, T, 24, par.data_ptr(), rows.data_ptr() + 8 * T, 24, None) == -1
            assert fx(h, rows.data_ptr(), 0, T, 24, par.data_ptr(), out.data_ptr(), 24, None) == 0
            assert fx(h, rows.data_ptr(), N, 0, 24, par.data_ptr(), out.data_ptr(), 24, None) == 0
    engine.synchronize()
    assert bool((out == SENT).all()) and bool((obj == SENT).all()) and bool((st == -77).all())
    assert bool((rows == 1.0).all()) and bool((par == .2).all())


# ---- the Python layer -------------------------------------------------------------------------------------------
def test_python_models(engine):
    from sparkts_amd import fit_ewma_partition, fit_garch_partition
    from sparkts_amd.models import EWMA, GARCH
    m = EWMA.fit_model(R.OIL)
    assert int(m.smoothing * 100.0) == 89 and m.smoothing == 0.8920138182337584
    orig = np.arange(1.0, 11.0)
    assert round(EWMA.EWMAModel(0.2).add_time_dependent_effects(orig)[-1], 2) == 6.54
    assert round(EWMA.EWMAModel(0.6).add_time_dependent_effects(orig)[-1], 2) == 9.33
    assert m.sse(R.OIL) == R.ewma_sse(R.OIL, m.smoothing) and m.gradient(R.OIL) == R.ewma_gradient(R.OIL, m.smoothing)
    dest = np.zeros(10)
    assert EWMA.EWMAModel(0.2).remove_time_dependent_effects(orig, dest) is dest
    _same(dest, np.array(R.ewma_remove(orig.tolist(), 0.2)))

    meta, arr = load_case("smallfit/garch_T97")
    ts = arr["series"][0]
    gm = GARCH.GARCHModel(.25, .35, .3)
    assert gm.log_likelihood(ts) == R.garch_loglik(ts.tolist(), .25, .35, .3)
    _same(gm.gradient(ts), np.array(R.garch_gradient(ts.tolist(), .25, .35, .3)))
    _same(gm.add_time_dependent_effects(ts), np.array(R.garch_add(ts.tolist(), .25, .35, .3)))
    _same(gm.remove_time_dependent_effects(ts), np.array(R.garch_remove(ts.tolist(), .25, .35, .3)))
    batch = GARCH.fit_models(arr["series"][:12])
    _same(batch.coefficients, arr["coef"][:12])
    for i in range(12):
        if arr["status"][i] == 0:
            one = GARCH.fit_model(arr["series"][i])
            _same(np.array([one.omega, one.alpha, one.beta]), arr["coef"][i])
        else:
            with pytest.raises(GARCH.ARIMAFitError) as e:
                GARCH.fit_model(arr["series"][i])
            assert e.value.status == arr["status"][i]
    meta, ea = load_case("smallfit/ewma_T75")
    eb = EWMA.fit_models(ea["series"][:12])
    _same(eb.smoothing, ea["coef"][:12, 0])
    for i in range(12):
        if ea["status"][i] == 0:
            assert EWMA.fit_model(ea["series"][i]).smoothing == ea["coef"][i, 0]
    with pytest.raises(EWMA.ARIMAFitError):
        eb.model(10)                                          # the NaN row ran to MaxEval
    # partition helpers: records of two lengths, input order kept
    recs = [(f"k{i}", arr["series"][i][: 97 if i % 2 else 60]) for i in range(6)]
    got = list(fit_garch_partition(recs, with_status=True))
    assert [k for k, _, _ in got] == [k for k, _ in recs]
    for i in (1, 3, 5):
        _same(got[i][1], arr["coef"][i])
        assert got[i][2] == arr["status"][i]
    eg = list(fit_ewma_partition([("a", ea["series"][0]), ("b", ea["series"][1])]))
    assert eg[0][0] == "a" and eg[0][1][0] == ea["coef"][0, 0] and eg[1][1][0] == ea["coef"][1, 0]


# ---- the JNI natives ----------------------------------------------------------------------------------------------
def test_jni_natives_match_direct_abi(engine):
    _vp, _i64, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    harness = os.path.join(ROOT, "tests", "jni_harness")
    subprocess.run(["make", "-s", "-C", harness], check=True)      # up to date after build(): a no-op
    lib = ctypes.CDLL(os.path.join(harness, "_build", "libjni_harness.so"))
    lib.fake_jni_env.restype = _vp
    fn = lambda name: getattr(lib, "Java_com_cloudera_sparkts_models_ArimaMI355XNative_00024_" + name)
    fn("create").restype = _i64
    fn("create").argtypes = [_vp, _vp, _i32]
    fn("destroy").argtypes = [_vp, _vp, _i64]
    for name in ("ewmaFitBatch", "garchFitBatch"):
        fn(name).argtypes = [_vp, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp]
    for name in ("ewmaRemoveEffectsBatch", "ewmaAddEffectsBatch", "garchRemoveEffectsBatch", "garchAddEffectsBatch"):
        fn(name).argtypes = [_vp, _vp, _i64, _vp, _i64, _i32, _vp, _vp]
    env = lib.fake_jni_env()
    p = lambda a: None if a is None else a.ctypes.data
    assert fn("ewmaFitBatch")(env, None, 0, None, 1, 4, None, None, None, None, None) == -1       # null handle
    h = fn("create")(env, None, 0)
    assert h != 0
    try:
        for model, name, native in (("ewma", "smallfit/ewma_T75", "ewmaFitBatch"),
                                    ("garch", "smallfit/garch_T97", "garchFitBatch")):
            meta, arr = load_case(name)
            N, T, K = 70, meta["T"], arr["coef"].shape[1]
            s = np.ascontiguousarray(arr["series"][:N])
            coef, obj = np.empty((N, K)), np.empty(N)
            st, ne, ng = np.empty(N, np.int32), np.empty(N, np.int32), np.empty(N, np.int32)
            assert fn(native)(env, None, h, p(s), N, T, p(coef), p(obj), p(st), p(ne), None) == 0
            _same(coef, arr["coef"][:N], native)
            _same(obj, arr["obj"][:N], native)
            _same(st, arr["status"][:N], native)
            _same(ne, arr["n_eval"][:N], native)
            par = np.ascontiguousarray(_params(N)[0 if model == "ewma" else 1])
            for d in ("Remove", "Add"):
                out = np.empty((N, T))
                assert fn(f"{model}{d}EffectsBatch")(env, None, h, p(s), N, T, p(par), p(out)) == 0
                _same(out, getattr(engine, f"{model}_{d.lower()}_effects")(s, par), model + d)
                assert fn(f"{model}{d}EffectsBatch")(env, None, h, p(s), N, T, p(par), p(s)) == -1
    finally:
        assert fn("destroy")(env, None, h) == 0
