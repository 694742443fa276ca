"""Measure the SURVEY.md 8(f) rows built this round on one GPU (device-resident inputs):
  forecast      ARIMAModel.forecast (k_forecast) on N x 1024 C2 series, nFuture=30, fitted coefficients
  order_search  C5 grid p,q in [0,5], d in [0,2], +-intercept (216 fits/series) on N x 1024 C2 series
  effects       (--effects, a run of its own) removeTimeDependentEffects / addTimeDependentEffects (k_effects) on
                N x 1024 C2 series with fitted (2,1,2)+c coefficients, against the forecast kernel with nFuture = 0 on
                the same batch: the launches alternate in one process, each timed with HIP events
  diag          (--diag, a run of its own) the residual diagnostics (k_diag: autocorr, dwtest, lbtest) on the
                (2,1,2)+c residuals of N x 1024 C2 series: diagnostics_device at max_lag 1, W, W + 1 and 20 and with
                only dwtest (one pass), residual_diagnostics_device at max_lag W, alternating with
                remove_effects_device on the same batch in one process, each launch timed with HIP events
  models        (--models, a run of its own) the small models (EWMA, GARCH(1,1); arima_models.hip) on N x 1024 rows: the
                four TimeSeriesModel-pair kernels against remove_effects_device at (2,1,2)+c on the same batch
                (alternating launches, HIP events), then the two fits with the fit kernel's round counters
Prints one JSON line. Also checks the device-pointer forecast against the host-buffer entry point on 64 rows.
usage: python tools/bench_next.py [--fc-series N] [--os-series N]
       python tools/bench_next.py --effects [--fx-series N] [--fx-launches K] [--out FILE]
       python tools/bench_next.py --diag [--fx-series N] [--fx-launches K] [--out FILE]
       python tools/bench_next.py --models [--fx-series N] [--fx-launches K] [--fit-launches K] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-timeseries_amd"))


def bench_effects(a):
    """remove / add against forecast(nFuture = 0): the same rows in, the same rows out (16 N T bytes), forecast doing
    strictly more work per element. Output rows are 128-B aligned (ld = T = 1024)."""
    import numpy as np
    import torch
    import sparkts_amd._lib as L
    from sparkts_amd import buildinfo
    eng = L.Engine.get(0)
    N, T, base = a.fx_series, 1024, [8.2, 0.2, 0.5, 0.3, 0.1]
    dev = torch.device("cuda:0")
    s = torch.empty((N, T), dtype=torch.float64, device=dev)
    eng.sample_device(s.data_ptr(), N, T, T, 2, 1, 2, True, base, 0.05, 20261015)
    coef = torch.empty((N, 5), dtype=torch.float64, device=dev)
    ll = torch.empty(N, dtype=torch.float64, device=dev)
    st = torch.empty(N, dtype=torch.int32, device=dev)
    eng.fit_batch_device(s.data_ptr(), N, T, T, 2, 1, 2, True, coef.data_ptr(), ll.data_ptr(), st.data_ptr())
    del ll, st
    o = torch.empty((N, T), dtype=torch.float64, device=dev)
    # a stream of the caller's, so that the HIP events bracket the launches (the null stream would select the
    # handle's own stream, and events recorded on torch's stream would time nothing)
    ts = torch.cuda.Stream()
    stream = ts.cuda_stream
    assert stream, "need a non-default stream"
    torch.cuda.synchronize()
    calls = {
        "forecast": lambda: eng.forecast_device(s.data_ptr(), N, T, T, 2, 1, 2, True, coef.data_ptr(), 0,
                                                o.data_ptr(), T, stream=stream, blocking=False),
        "remove": lambda: eng.remove_effects_device(s.data_ptr(), N, T, T, 2, 1, 2, True, coef.data_ptr(),
                                                    o.data_ptr(), T, stream=stream, blocking=False),
        "add": lambda: eng.add_effects_device(s.data_ptr(), N, T, T, 2, 1, 2, True, coef.data_ptr(), o.data_ptr(), T,
                                              stream=stream, blocking=False),
    }
    for _ in range(3):                                       # warm-up: every kernel loaded, clocks up
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in calls}
    for _ in range(max(a.fx_launches, 20)):                  # alternating launches, one HIP event pair each
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            f()
            e1.record(ts)
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {"gpu": torch.cuda.get_device_name(0), "series": N, "T": T, "order": "(2,1,2)+c",
           "launches_each": len(ev["forecast"]), "bytes_per_launch": 16 * N * T,
           "library_sha": buildinfo.library_sha(), "source_sha": buildinfo.source_sha()}
    for k, pairs in ev.items():
        ms = np.array([e0.elapsed_time(e1) for e0, e1 in pairs])
        med = float(np.median(ms))
        out[k] = {"median_ms": med, "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                  "bytes_per_s": 16.0 * N * T / (med * 1e-3), "series_per_s": N / (med * 1e-3)}
    bound = out["forecast"]["median_ms"] + (out["forecast"]["max_ms"] - out["forecast"]["min_ms"])
    out["bound_ms"] = bound                                  # forecast's median + its spread in this run
    out["remove_within_bound"] = bool(out["remove"]["median_ms"] <= bound)
    out["add_within_bound"] = bool(out["add"]["median_ms"] <= bound)
    # the timed kernels computed the host entry point's bits (the last launch was add)
    host = eng.add_effects(s[:64].cpu().numpy(), 2, 1, 2, True, coef[:64].cpu().numpy())
    out["device_vs_host_api_identical"] = bool(np.array_equal(host, o[:64].cpu().numpy(), equal_nan=True))
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


def bench_diag(a):
    """diagnostics_device with max_lag <= W reads the rows twice (16 N T bytes), remove_effects_device reads and
    writes them once each (the same bytes): the expectation is the diagnostics median within remove's median plus
    remove's spread (max - min) in this run. Every further group of W lags is one more pass pair."""
    import numpy as np
    import torch
    import sparkts_amd._lib as L
    from sparkts_amd import buildinfo
    eng = L.Engine.get(0)
    W = 8                                                    # kDgW (csrc/arima_launch.hpp)
    N, T, base = a.fx_series, 1024, [8.2, 0.2, 0.5, 0.3, 0.1]
    dev = torch.device("cuda:0")
    s = torch.empty((N, T), dtype=torch.float64, device=dev)
    eng.sample_device(s.data_ptr(), N, T, T, 2, 1, 2, True, base, 0.05, 20261015)
    coef = torch.empty((N, 5), dtype=torch.float64, device=dev)
    ll = torch.empty(N, dtype=torch.float64, device=dev)
    st = torch.empty(N, dtype=torch.int32, device=dev)
    eng.fit_batch_device(s.data_ptr(), N, T, T, 2, 1, 2, True, coef.data_ptr(), ll.data_ptr(), st.data_ptr())
    del ll, st
    r = torch.empty((N, T), dtype=torch.float64, device=dev)     # the residuals the diagnostics read
    o = torch.empty((N, T), dtype=torch.float64, device=dev)     # the timed remove launches write here
    eng.remove_effects_device(s.data_ptr(), N, T, T, 2, 1, 2, True, coef.data_ptr(), r.data_ptr(), T)
    acf = torch.empty((N, 20), dtype=torch.float64, device=dev)
    dw, lbs, lbp = (torch.empty(N, dtype=torch.float64, device=dev) for _ in range(3))
    ts = torch.cuda.Stream()                                 # see bench_effects
    stream = ts.cuda_stream
    assert stream, "need a non-default stream"
    torch.cuda.synchronize()

    def diag(lag):
        return lambda: eng.diagnostics_device(r.data_ptr(), N, T, T, lag, acf.data_ptr(), dw.data_ptr(),
                                              lbs.data_ptr(), lbp.data_ptr(), stream=stream, blocking=False)

    calls = {
        "remove": lambda: eng.remove_effects_device(s.data_ptr(), N, T, T, 2, 1, 2, True, coef.data_ptr(),
                                                    o.data_ptr(), T, stream=stream, blocking=False),
        "dw_only": lambda: eng.diagnostics_device(r.data_ptr(), N, T, T, 0, None, dw.data_ptr(), None, None,
                                                  stream=stream, blocking=False),
        "diag_lag1": diag(1), f"diag_lag{W}": diag(W), f"diag_lag{W + 1}": diag(W + 1), "diag_lag20": diag(20),
        f"residual_diag_lag{W}": lambda: eng.residual_diagnostics_device(
            s.data_ptr(), N, T, T, 2, 1, 2, True, coef.data_ptr(), W, acf.data_ptr(), dw.data_ptr(), lbs.data_ptr(),
            lbp.data_ptr(), stream=stream, blocking=False),
    }
    for _ in range(3):                                       # warm-up: every kernel loaded, workspace allocated
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in calls}
    for _ in range(max(a.fx_launches, 20)):                  # alternating launches, one HIP event pair each
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            f()
            e1.record(ts)
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {"gpu": torch.cuda.get_device_name(0), "series": N, "T": T, "order": "(2,1,2)+c", "W": W,
           "launches_each": len(ev["remove"]), "bytes_per_pass_pair": 16 * N * T,
           "library_sha": buildinfo.library_sha(), "source_sha": buildinfo.source_sha()}
    for k, pairs in ev.items():
        ms = np.array([e0.elapsed_time(e1) for e0, e1 in pairs])
        out[k] = {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}
    bound = out["remove"]["median_ms"] + (out["remove"]["max_ms"] - out["remove"]["min_ms"])
    out["bound_ms"] = bound                                  # remove's median + its spread in this run
    for k in ("diag_lag1", f"diag_lag{W}"):
        out[k + "_within_bound"] = bool(out[k]["median_ms"] <= bound)
    # the last timed launch's outputs equal the host entry point's on the first 64 rows
    host = eng.residual_diagnostics(s[:64].cpu().numpy(), 2, 1, 2, True, coef[:64].cpu().numpy(), W)
    out["device_vs_host_api_identical"] = bool(
        np.array_equal(host["acf"], acf.view(-1)[:64 * W].view(64, W).cpu().numpy(), equal_nan=True)
        and np.array_equal(host["lb_stat"], lbs[:64].cpu().numpy(), equal_nan=True)
        and np.array_equal(host["dw"], dw[:64].cpu().numpy(), equal_nan=True))
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


def bench_models(a):
    """The small models, device-resident, f64. Effects: the four k_model_effects instances move the bytes of
    remove_effects_device at (2,1,2)+c (16 N T) with less arithmetic, so the expectation is each median within that
    call's median plus its spread (max - min) in this run. Fits: no expectation -- ms, series/s and the round counters
    (wave passes, the slowest wave's passes, the live-lane fraction, the rate passes x 64 x T x 8 B / time)."""
    import numpy as np
    import torch
    import sparkts_amd._lib as L
    from sparkts_amd import buildinfo
    eng = L.Engine.get(0)
    N, T = a.fx_series, 1024
    dev = torch.device("cuda:0")
    torch.manual_seed(20261019)
    gpar = torch.tensor([.2, .3, .5], dtype=torch.float64, device=dev).repeat(N, 1).contiguous()
    epar = torch.full((N, 1), 0.9, dtype=torch.float64, device=dev)
    acoef = torch.tensor([8.2, 0.2, 0.5, 0.3, 0.1], dtype=torch.float64, device=dev).repeat(N, 1).contiguous()
    noise = torch.randn((N, T), dtype=torch.float64, device=dev)
    g = torch.empty((N, T), dtype=torch.float64, device=dev)     # GARCH(.2, .3, .5) rows: the model over N(0, 1)
    torch.cuda.synchronize()                                     # the engine's stream does not wait for torch's: randn done
    eng.model_effects_device("garch", "add", noise.data_ptr(), N, T, T, gpar.data_ptr(), g.data_ptr(), T)
    o = noise                                                    # the timed effects launches write here
    ts = torch.cuda.Stream()                                     # see bench_effects
    stream = ts.cuda_stream
    assert stream, "need a non-default stream"
    torch.cuda.synchronize()

    def fx(model, direction, par):
        return lambda: eng.model_effects_device(model, direction, g.data_ptr(), N, T, T, par.data_ptr(), o.data_ptr(),
                                                T, stream=stream, blocking=False)

    calls = {
        "arima_remove": lambda: eng.remove_effects_device(g.data_ptr(), N, T, T, 2, 1, 2, True, acoef.data_ptr(),
                                                          o.data_ptr(), T, stream=stream, blocking=False),
        "ewma_remove": fx("ewma", "remove", epar), "ewma_add": fx("ewma", "add", epar),
        "garch_remove": fx("garch", "remove", gpar), "garch_add": fx("garch", "add", gpar),
    }
    for _ in range(3):                                           # warm-up: every kernel loaded, clocks up
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in calls}
    for _ in range(max(a.fx_launches, 20)):                      # alternating launches, one HIP event pair each
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            f()
            e1.record(ts)
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {"gpu": torch.cuda.get_device_name(0), "series": N, "T": T, "launches_each": len(ev["arima_remove"]),
           "bytes_per_effects_launch": 16 * N * T, "library_sha": buildinfo.library_sha(),
           "source_sha": buildinfo.source_sha(), "effects": {}, "fits": {}}
    for k, pairs in ev.items():
        ms = np.array([e0.elapsed_time(e1) for e0, e1 in pairs])
        med = float(np.median(ms))
        out["effects"][k] = {"median_ms": med, "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                             "bytes_per_s": 16.0 * N * T / (med * 1e-3)}
    ref = out["effects"]["arima_remove"]
    out["effects"]["bound_ms"] = ref["median_ms"] + (ref["max_ms"] - ref["min_ms"])
    for k in ("ewma_remove", "ewma_add", "garch_remove", "garch_add"):
        out["effects"][k]["within_bound"] = bool(out["effects"][k]["median_ms"] <= out["effects"]["bound_ms"])
    print(json.dumps({"progress": "effects", **out["effects"]}), file=sys.stderr, flush=True)
    # the last timed launch (garch add) equals the host entry point on the first 64 rows
    host = eng.garch_add_effects(g[:64].cpu().numpy(), (.2, .3, .5))
    out["device_vs_host_api_identical"] = bool(np.array_equal(host, o[:64].cpu().numpy(), equal_nan=True))

    # fits: EWMA on random walks, GARCH on the rows above
    torch.cumsum(torch.randn((N, T), dtype=torch.float64, device=dev), dim=1, out=o)
    torch.cuda.synchronize()                                     # the walks are complete before a fit on another stream reads them
    par = torch.empty((N, 3), dtype=torch.float64, device=dev)
    obj = torch.empty(N, dtype=torch.float64, device=dev)
    st, ne, ng = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(3))
    for model, rows in (("ewma", o), ("garch", g)):
        fit = eng.ewma_fit_batch_device if model == "ewma" else eng.garch_fit_batch_device
        ms = []
        for i in range(1 + max(a.fit_launches, 1)):              # the first launch is the warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            fit(rows.data_ptr(), N, T, T, par.data_ptr(), obj.data_ptr(), st.data_ptr(), ne.data_ptr(), ng.data_ptr(),
                stream=stream, blocking=False)
            e1.record(ts)
            torch.cuda.synchronize()
            if i:
                ms.append(e0.elapsed_time(e1))
            print(json.dumps({"progress": model, "launch": i, "ms": e0.elapsed_time(e1)}), file=sys.stderr, flush=True)
        ms = np.array(ms)
        med = float(np.median(ms))
        c = eng.model_fit_stats()
        stn, nev = st.cpu().numpy(), ne.cpu().numpy()
        ok = stn == 0
        zero_rows = int((rows == 0).all(dim=1).sum())            # guards the inputs: an unfinished row would be all zero
        out["fits"][model] = {
            "all_zero_input_rows": zero_rows,
            "median_ms": med, "min_ms": float(ms.min()), "max_ms": float(ms.max()), "launches": len(ms),
            "series_per_s": N / (med * 1e-3), "wave_passes": c["wave_passes"], "lane_passes": c["lane_passes"],
            "max_wave_passes": c["max_wave_passes"], "mean_wave_passes": c["wave_passes"] / ((N + 63) // 64),
            "live_lane_fraction": c["lane_passes"] / (64.0 * c["wave_passes"]),
            "tile_rate_bytes_per_s": c["wave_passes"] * 64.0 * T * 8 / (med * 1e-3),
            "live_row_bytes_per_s": c["lane_passes"] * 1.0 * T * 8 / (med * 1e-3),
            "status_counts": {str(k): int(v) for k, v in zip(*np.unique(stn, return_counts=True))},
            "n_eval_ok_median": float(np.median(nev[ok])) if ok.any() else None,
            "n_eval_ok_p99": float(np.percentile(nev[ok], 99)) if ok.any() else None,
            "n_eval_ok_max": int(nev[ok].max()) if ok.any() else None}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", action="store_true", help="measure the EWMA / GARCH effects kernels and fits, only")
    ap.add_argument("--fit-launches", type=int, default=3, help="--models: timed launches of each fit")
    ap.add_argument("--diag", action="store_true", help="measure the residual diagnostics against remove effects, only")
    ap.add_argument("--effects", action="store_true", help="measure remove / add effects against forecast, only")
    ap.add_argument("--fx-series", type=int, default=1 << 20)
    ap.add_argument("--fx-launches", type=int, default=20)
    ap.add_argument("--out", default=None, help="--effects / --diag: also write the JSON line to this file")
    ap.add_argument("--fc-series", type=int, default=1 << 20)
    ap.add_argument("--os-series", type=int, default=1 << 16)
    ap.add_argument("--n-future", type=int, default=30)
    a = ap.parse_args()
    if a.models:
        bench_models(a)
        return
    if a.effects:
        bench_effects(a)
        return
    if a.diag:
        bench_diag(a)
        return
    import numpy as np
    import torch
    import sparkts_amd._lib as L
    eng = L.Engine.get(0)
    T, base = 1024, [8.2, 0.2, 0.5, 0.3, 0.1]
    dev = torch.device("cuda:0")
    out = {"gpu": torch.cuda.get_device_name(0)}

    # forecast: fit first (coefficients resident in HBM), then time the forecast kernel alone
    N = a.fc_series
    s = torch.empty((N, T), dtype=torch.float64, device=dev)
    eng.sample_device(s.data_ptr(), N, T, T, 2, 1, 2, True, base, 0.05, 20261015)
    coef = torch.empty((N, 5), dtype=torch.float64, device=dev)
    ll = torch.empty(N, dtype=torch.float64, device=dev)
    st = torch.empty(N, dtype=torch.int32, device=dev)
    eng.fit_batch_device(s.data_ptr(), N, T, T, 2, 1, 2, True, coef.data_ptr(), ll.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    L_ = T + a.n_future
    LD = (L_ + 15) // 16 * 16            # 128-B aligned output rows: k_forecast's flushes are whole lines
    fo = torch.empty((N, LD), dtype=torch.float64, device=dev)
    eng.forecast_device(s.data_ptr(), N, T, T, 2, 1, 2, True, coef.data_ptr(), a.n_future, fo.data_ptr(), LD)
    torch.cuda.synchronize()
    reps = 5
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.forecast_device(s.data_ptr(), N, T, T, 2, 1, 2, True, coef.data_ptr(), a.n_future, fo.data_ptr(), LD)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    host = eng.forecast(s[:64].cpu().numpy(), 2, 1, 2, True, coef[:64].cpu().numpy(), a.n_future)
    same = bool(np.array_equal(host, fo[:64, :L_].cpu().numpy()))
    bytes_ = N * (T * 8 + 5 * 8 + L_ * 8)
    out["forecast"] = {"series": N, "T": T, "n_future": a.n_future, "ms": dt * 1e3, "series_per_s": N / dt,
                       "algorithmic_GBps": bytes_ / dt / 1e9, "device_vs_host_api_identical": same}
    del s, coef, ll, st, fo
    torch.cuda.empty_cache()

    # order search (C5 grid)
    N = a.os_series
    if N <= 0:
        print(json.dumps(out))
        return
    s = torch.empty((N, T), dtype=torch.float64, device=dev)
    eng.sample_device(s.data_ptr(), N, T, T, 2, 1, 2, True, base, 0.05, 20261015)
    order = torch.empty((N, 4), dtype=torch.int32, device=dev)
    cbest = torch.empty((N, 11), dtype=torch.float64, device=dev)
    aic = torch.empty(N, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.order_search_device(s.data_ptr(), N, T, T, 5, 2, 5, 2, order.data_ptr(), cbest.data_ptr(), aic.data_ptr())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    o = order.cpu().numpy()
    sel = {}
    for r in o:
        key = f"({r[0]},{r[1]},{r[2]}){'+c' if r[3] == 1 else ''}" if r[0] >= 0 else "none"
        sel[key] = sel.get(key, 0) + 1
    top = dict(sorted(sel.items(), key=lambda kv: -kv[1])[:6])
    out["order_search"] = {"series": N, "T": T, "grid_fits_per_series": 216, "s": dt, "series_per_s": N / dt,
                           "fits_per_s": N * 216 / dt, "selected_orders_top": top}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
