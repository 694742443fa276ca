"""arima_get_last_stats after every kind of fit call: a device fit recorded in its context (css-cgd with and without
user inits, the AR-only shortcut, css-bobyqa), a device fit cut into slices (one slice, two with a tail of one row, more
slices than the ring has slots, at fit_pipeline 1 and 3), the order search (one lane and eight), and which call the stats
belong to after calls of different kinds. What is asserted follows from the inputs alone -- series counts, the sums of
the per-series evaluation counts, the Hannan-Rissanen pass formula, the SURVEY 8(d) flops formula recomputed from the
same stats' pass counters -- so the file holds for any build that keeps the stats' meaning. All rows come from the
device sampler with fixed seeds. The CPU side (the stats functions against the bodies they replaced) is
tests/test_fitstats_sim.py."""
import numpy as np
import pytest

import sparkts_amd._lib as L

pytestmark = pytest.mark.gpu

CGD, BOBYQA = L.METHOD_CSS_CGD, L.METHOD_CSS_BOBYQA
OUT_KEYS = ("coef", "ll", "status", "n_eval", "n_grad", "flags")
# counter-backed fields that are zero when no css-cgd kernel ran
COUNTERS = ("f_passes", "g_passes", "n_eval", "n_grad", "wave_f_passes", "wave_g_passes", "spec_hits",
            "wave_multi_passes", "spec_chains", "ride_passes", "express_series", "express_f_passes", "express_g_passes",
            "express_pit_passes", "express_pit_sweeps", "express_pit_g_passes", "wave_chains", "low_util_passes",
            "merge_series", "merge_waves")
_CACHE = {}


def _rows(engine, N, T, p, d, q, base, seed):
    import torch
    key = (N, T, p, d, q, seed)
    if key not in _CACHE:
        buf = torch.empty((max(N, 1), T), dtype=torch.float64, device="cuda")
        engine.sample_device(buf.data_ptr(), N, T, T, p, d, q, 1, base, 0.05, seed, 0)
        _CACHE[key] = buf
    return _CACHE[key]


def _device_fit(engine, rows, N, T, p, d, q, I, method=CGD, user_init=None, take_stats=True):
    """One arima_fit_batch_device call: its six outputs as numpy arrays and (take_stats) its stats."""
    import torch
    k = p + q + I
    dev = rows.device
    out = dict(coef=torch.full((max(N, 1), max(k, 1)), -7.25, dtype=torch.float64, device=dev),
               ll=torch.empty(max(N, 1), dtype=torch.float64, device=dev),
               status=torch.empty(max(N, 1), dtype=torch.int32, device=dev),
               n_eval=torch.empty(max(N, 1), dtype=torch.int32, device=dev),
               n_grad=torch.empty(max(N, 1), dtype=torch.int32, device=dev),
               flags=torch.empty(max(N, 1), dtype=torch.uint8, device=dev))
    ui = None
    if user_init is not None:
        ui = torch.tensor(np.broadcast_to(np.asarray(user_init, dtype=np.float64), (N, k)).copy(), device=dev)
    engine.fit_batch_device(rows.data_ptr(), N, T, T, p, d, q, I, out["coef"].data_ptr(), out["ll"].data_ptr(),
                            out["status"].data_ptr(), out["n_eval"].data_ptr(), out["n_grad"].data_ptr(),
                            out["flags"].data_ptr(), d_user_init=ui.data_ptr() if ui is not None else None,
                            method=method)
    st = engine.stats() if take_stats else None
    return {key: v.cpu().numpy()[:N] for key, v in out.items()}, st


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))
    return np.array_equal(a, b)


def _flops(st, N, n, p, q, I, with_hr):
    """U S (2(p+q)+4) + G S (2(p+q)+4 + 2kq + 1+p+q + 2k) + W_HR from the stats' own pass counters, in exact
    integer arithmetic."""
    k, M = I + p + q, max(p, q)
    m = M + 1
    S = max(n - M, 0)
    ff = 2 * (p + q) + 4
    fg = ff + 2 * k * q + 1 + p + q + 2 * k
    U = st["f_passes"] + st["ride_passes"] + st["express_f_passes"] + st["spec_hits"]
    G = st["g_passes"] - st["ride_passes"] + st["express_g_passes"]
    whr = N * (3 * max(n - m, 0) * (m + 1) ** 2 + 3 * max(n - 2 * M - 1, 0) * k * k + 2 * max(n - m, 0) * m)
    return U * S * ff + G * S * fg + (whr if with_hr else 0)


def _flops_match(st, want):
    # a dozen double roundings of non-negative terms: within 2e-15 relative; a wrong term is far outside 1e-12
    print(f"flops {st['flops']!r} formula {want}")
    assert want > 0 and abs(st["flops"] - want) <= 1e-12 * want, (st["flops"], want)


C2_BASE = [8.2, 0.2, 0.5, 0.3, 0.1]
N1, T1 = 130, 64            # two full waves of 64 series and a tail of two


# ---- 1-4. a device fit recorded in its context ----------------------------------------------------------------------
@pytest.mark.parametrize("user_init", [False, True])
def test_unsliced_cgd_fit_stats(engine, user_init):
    p, d, q, I = 2, 1, 2, 1
    k, m = 5, 3
    rows = _rows(engine, N1, T1, p, d, q, C2_BASE, 20261020)
    res, st = _device_fit(engine, rows, N1, T1, p, d, q, I, user_init=C2_BASE if user_init else None)
    print(st)
    assert st["n_series"] == st["series_done"] == N1
    assert st["n_eval"] == int(res["n_eval"].sum(dtype=np.int64)) > 0
    assert st["n_grad"] == int(res["n_grad"].sum(dtype=np.int64)) > 0
    assert st["fault"] == 0 and st["fault_info"] == [0] * 5
    assert st["hr_passes"] == (0 if user_init else N1 * (2 * (1 + m) - 1 + 2 * k - I))
    _flops_match(st, _flops(st, N1, T1 - d, p, q, I, with_hr=not user_init))
    assert st["ms_total"] >= st["ms_cg_fit"] > 0
    assert engine.stats() == st


def test_ar_only_device_fit_stats(engine):
    p, d, q, I = 2, 0, 0, 1
    rows = _rows(engine, N1, T1, 2, 1, 2, C2_BASE, 20261020)
    res, st = _device_fit(engine, rows, N1, T1, p, d, q, I)
    print(st)
    assert all(st[name] == 0 for name in COUNTERS), st
    assert st["n_series"] == st["series_done"] == N1 and st["fault"] == 0
    assert st["hr_passes"] == N1 * (2 * (I + p) - I)
    # today's value: a device fit counts the Hannan-Rissanen term for the AR-only shortcut too (one OLS runs instead);
    # the order search leaves it out for its AR-only grid points
    _flops_match(st, _flops(st, N1, T1, p, q, I, with_hr=True))
    assert engine.stats() == st


def test_bobyqa_device_fit_stats(engine):
    rows = _rows(engine, N1, T1, 2, 1, 2, C2_BASE, 20261020)
    res, st = _device_fit(engine, rows, N1, T1, 2, 1, 2, 1, method=BOBYQA)
    print(st)
    assert st["n_series"] == st["series_done"] == N1
    assert st["n_eval"] == 0 and st["fault"] == 0          # css-bobyqa keeps no device counters
    assert engine.stats() == st


# ---- 5. slices ------------------------------------------------------------------------------------------------------
T5 = 16


def _whole_fit(engine, N):
    """The reference of the slice cases: the same fit as one slice (default slice size), computed once per N."""
    key = ("whole", N)
    if key not in _CACHE:
        assert engine.get_option("fit_slice_bytes") == 0
        rows = _rows(engine, N, T5, 1, 0, 1, [1.0, 0.4, 0.3], 77)
        _CACHE[key] = _device_fit(engine, rows, N, T5, 1, 0, 1, 1)
    return _CACHE[key]


@pytest.mark.parametrize("pipeline", [1, 3])
@pytest.mark.parametrize("N", [1024, 1025, 67589])     # one slice; two, a tail of one row; 67 slices > the 64 slots
def test_sliced_fit_stats_cover_every_slice(engine, N, pipeline):
    # (67 slices are 67 launches, each as long as its slowest series, about 170 ms whatever the sampler's settings:
    # 12 s at fit_pipeline 1, 6 s at 3; the other cases take under half a second)
    whole, st_whole = _whole_fit(engine, N)
    rows = _rows(engine, N, T5, 1, 0, 1, [1.0, 0.4, 0.3], 77)
    prev = engine.get_option("fit_pipeline")
    try:
        engine.set_option("fit_pipeline", pipeline)
        engine.set_option("fit_slice_bytes", 1)            # the smallest slice: 1024 series
        res, st = _device_fit(engine, rows, N, T5, 1, 0, 1, 1)
        again = engine.stats()
    finally:
        engine.set_option("fit_slice_bytes", 0)
        engine.set_option("fit_pipeline", prev)
    print(st)
    for key in OUT_KEYS:
        assert _same(res[key], whole[key]), key
    assert st["n_series"] == st["series_done"] == N
    assert st_whole["n_series"] == st_whole["series_done"] == N
    for name in ("n_eval", "n_grad", "hr_passes"):
        assert st[name] == st_whole[name] > 0, name
    assert st["n_eval"] == int(res["n_eval"].sum(dtype=np.int64))
    assert st["fault"] == 0
    assert again == st


# ---- 6. the order search --------------------------------------------------------------------------------------------
N6, T6 = 70, 48


def _search(engine, rows, N, T, max_p, max_d, max_q, mode):
    import torch
    order = torch.empty((N, 4), dtype=torch.int32, device=rows.device)
    coef = torch.empty((N, 11), dtype=torch.float64, device=rows.device)
    aic = torch.empty(N, dtype=torch.float64, device=rows.device)
    engine.order_search_device(rows.data_ptr(), N, T, T, max_p, max_d, max_q, mode, order.data_ptr(), coef.data_ptr(),
                               aic.data_ptr())
    return engine.stats()


def _grid_point_sums(engine, rows):
    """n_eval and n_grad of a device fit of every grid point of bounds (1,1,1), intercept mode 2, summed."""
    if "grid" not in _CACHE:
        ne = ng = 0
        for d in (0, 1):
            for p in (0, 1):
                for q in (0, 1):
                    for I in (0, 1):
                        _, st = _device_fit(engine, rows, N6, T6, p, d, q, I)
                        cgd = not (p > 0 and q == 0) and p + q + I > 0
                        assert (st["n_eval"] > 0) == cgd, (p, d, q, I, st)    # AR-only and zero-parameter points: zero
                        ne += st["n_eval"]
                        ng += st["n_grad"]
        _CACHE["grid"] = (ne, ng)
    return _CACHE["grid"]


@pytest.mark.parametrize("lanes", [1, 8])
def test_order_search_stats(engine, lanes):
    rows = _rows(engine, N6, T6, 1, 1, 1, [0.5, 0.4, 0.3], 4242)
    ne, ng = _grid_point_sums(engine, rows)
    prev = engine.get_option("search_lanes")
    try:
        engine.set_option("search_lanes", lanes)
        st = _search(engine, rows, N6, T6, 1, 1, 1, 2)
        again = engine.stats()
        one = _search(engine, rows, N6, T6, 0, 0, 0, 1)        # one grid point: (0,0,0)+c
    finally:
        engine.set_option("search_lanes", prev)
    print(st)
    assert st["n_series"] == st["series_done"] == 16 * N6
    assert st["n_eval"] == ne and st["n_grad"] == ng
    assert st["hr_passes"] == 0
    assert st["ms_total"] == st["ms_cg_fit"] > 0
    assert st["fault"] == 0
    assert again == st
    assert one["n_series"] == one["series_done"] == N6
    _flops_match(one, _flops(one, N6, T6, 0, 0, 1, with_hr=True))


# ---- 7. which call the stats belong to ------------------------------------------------------------------------------
def test_stats_follow_the_last_fit_call(engine):
    rows = _rows(engine, N6, T6, 1, 1, 1, [0.5, 0.4, 0.3], 4242)
    fit_rows = _rows(engine, N1, T1, 2, 1, 2, C2_BASE, 20261020)
    _, ref = _device_fit(engine, fit_rows, N1, T1, 2, 1, 2, 1)
    fixed = ("n_series", "series_done", "n_eval", "n_grad", "hr_passes", "fault")   # independent of the schedule
    # a search, then a fit: the fit's
    import torch
    order = torch.empty((N6, 4), dtype=torch.int32, device=rows.device)
    coef = torch.empty((N6, 11), dtype=torch.float64, device=rows.device)
    aic = torch.empty(N6, dtype=torch.float64, device=rows.device)
    engine.order_search_device(rows.data_ptr(), N6, T6, T6, 1, 1, 1, 2, order.data_ptr(), coef.data_ptr(),
                               aic.data_ptr())
    _, st = _device_fit(engine, fit_rows, N1, T1, 2, 1, 2, 1)
    assert {f: st[f] for f in fixed} == {f: ref[f] for f in fixed}
    # a fit, then a call that is no fit, then the stats: still the fit's
    _device_fit(engine, fit_rows, N1, T1, 2, 1, 2, 1, take_stats=False)
    engine.kpss(rows.cpu().numpy())
    st = engine.stats()
    assert {f: st[f] for f in fixed} == {f: ref[f] for f in fixed}
    assert st["ms_total"] >= st["ms_cg_fit"] > 0
    # an empty fit: zeros
    _, st = _device_fit(engine, fit_rows, 0, T1, 2, 1, 2, 1)
    assert all(x == 0 for v in st.values() for x in (v if isinstance(v, list) else [v])), st
