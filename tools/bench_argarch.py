"""Measure the fused ARGARCH fit against the GARCH fit of precomputed residual rows on one GPU (device-resident, f64).

  rows      N x 1024 series of ARGARCHModel(.5, .4, .2, .3, .5) driven by N(0, 1) (the add-effects kernel)
  baseline  arima_garch_fit_batch_device on the AR(1) residual rows of the same data (arima_fit_batch_device(1, 0, 0,
            intercept), then arima_ar_remove_effects_batch_device: bit-identical to what the fused fit forms in its passes)
  new       arima_argarch_fit_batch_device on the raw rows
  ar_stage  arima_fit_batch_device(1, 0, 0, intercept) alone: the kernel the fused call launches first
The three alternate in one process after a warm-up launch of each, every launch timed with a HIP event pair; medians
and spreads (max - min) are reported. The round counters of the two fits must be equal (the trajectories are
bit-identical); the expectation checked is
  new median <= baseline median + baseline spread + baseline median * ar_passes / baseline max_wave_passes
with ar_passes = 5 passes over a row: 2 per column of the streamed Householder least squares (2 columns: intercept, lag)
and the CSS pass of the AR path. Prints one JSON line.
usage: python tools/bench_argarch.py [--series N] [--launches K] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-timeseries_amd"))

AR_PASSES = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=1 << 16)
    ap.add_argument("--launches", type=int, default=5, help="timed launches of each call (at least 5)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    import numpy as np
    import torch
    import sparkts_amd._lib as L
    from sparkts_amd import buildinfo
    eng = L.Engine.get(0)
    N, T = a.series, 1024
    dev = torch.device("cuda:0")
    torch.manual_seed(20261020)
    f64 = dict(dtype=torch.float64, device=dev)
    mpar = torch.tensor([.5, .4, .2, .3, .5], **f64).repeat(N, 1).contiguous()
    noise = torch.randn((N, T), **f64)
    raw, res = torch.empty((N, T), **f64), torch.empty((N, T), **f64)
    ar_coef, ar_ll = torch.empty((N, 2), **f64), torch.empty(N, **f64)
    ar_st = torch.empty(N, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()                                     # the engine's stream does not wait for torch's
    eng.model_effects_device("argarch", "add", noise.data_ptr(), N, T, T, mpar.data_ptr(), raw.data_ptr(), T)
    eng.fit_batch_device(raw.data_ptr(), N, T, T, 1, 0, 0, True, ar_coef.data_ptr(), ar_ll.data_ptr(), ar_st.data_ptr())
    eng.ar_effects_device("remove", raw.data_ptr(), N, T, T, 1, ar_coef.data_ptr(), res.data_ptr(), T)
    assert int((ar_st != 0).sum()) == 0, "an AR stage failed on generated rows"
    ts = torch.cuda.Stream()
    stream = ts.cuda_stream
    assert stream, "need a non-default stream"
    out5, out3, obj = torch.empty((N, 5), **f64), torch.empty((N, 3), **f64), torch.empty(N, **f64)
    ints = {k: [torch.empty(N, dtype=torch.int32, device=dev) for _ in range(3)] for k in ("garch", "argarch")}
    ar_out = (torch.empty((N, 2), **f64), torch.empty(N, **f64), torch.empty(N, dtype=torch.int32, device=dev))
    calls = {
        "garch_on_residuals": lambda: eng.garch_fit_batch_device(
            res.data_ptr(), N, T, T, out3.data_ptr(), obj.data_ptr(), *(t.data_ptr() for t in ints["garch"]),
            stream=stream, blocking=False),
        "argarch_fused": lambda: eng.argarch_fit_batch_device(
            raw.data_ptr(), N, T, T, out5.data_ptr(), obj.data_ptr(), *(t.data_ptr() for t in ints["argarch"]),
            stream=stream, blocking=False),
        "ar_stage": lambda: eng.fit_batch_device(raw.data_ptr(), N, T, T, 1, 0, 0, True, ar_out[0].data_ptr(),
                                                 ar_out[1].data_ptr(), ar_out[2].data_ptr(), stream=stream,
                                                 blocking=False),
    }
    ms = {k: [] for k in calls}
    counters = {}
    for i in range(1 + max(a.launches, 5)):                      # launch 0 of each is the warm-up
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            f()
            e1.record(ts)
            torch.cuda.synchronize()
            if k != "ar_stage":
                counters[k] = eng.model_fit_stats()
            if i:
                ms[k].append(e0.elapsed_time(e1))
            print(json.dumps({"progress": k, "launch": i, "ms": e0.elapsed_time(e1)}), file=sys.stderr, flush=True)
    out = {"gpu": torch.cuda.get_device_name(0), "series": N, "T": T, "launches_each": len(ms["argarch_fused"]),
           "library_sha": buildinfo.library_sha(), "source_sha": buildinfo.source_sha(), "ar_passes": AR_PASSES}
    for k, v in ms.items():
        v = np.array(v)
        out[k] = {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()),
                  "spread_ms": float(v.max() - v.min()), "series_per_s": N / (float(np.median(v)) * 1e-3)}
    for k, c in counters.items():
        out[k].update(wave_passes=c["wave_passes"], lane_passes=c["lane_passes"], max_wave_passes=c["max_wave_passes"])
    st = ints["argarch"][0].cpu().numpy()
    out["argarch_fused"]["status_counts"] = {str(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))}
    base, new = out["garch_on_residuals"], out["argarch_fused"]
    out["counters_equal"] = bool(counters["garch_on_residuals"] == counters["argarch_fused"])
    same = lambda x, y: bool(np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True))
    out["results_identical"] = bool(same(out5[:, 2:], out3) and same(out5[:, :2], ar_out[0]) and
                                    all(same(x, y) for x, y in zip(ints["garch"], ints["argarch"])))
    out["ar_share_by_passes"] = AR_PASSES / base["max_wave_passes"]
    out["bound_ms"] = base["median_ms"] + base["spread_ms"] + base["median_ms"] * out["ar_share_by_passes"]
    out["fused_minus_baseline_ms"] = new["median_ms"] - base["median_ms"]
    out["within_bound"] = bool(new["median_ms"] <= out["bound_ms"])
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
