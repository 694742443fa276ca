"""Measure the batched ARIMAX fit on one GPU (device-resident, f64) at N x 1024, ARIMAX(1,1,1) with k = 2 regressor
columns, xregMaxLag 1 and the original columns (K' = 7 coefficients):

  arimax_shared      arima_arimax_fit_batch_device, one regressor matrix shared by every series
  arimax_per_series  the same with one regressor matrix per series
  arima              arima_fit_batch_device at (1,1,1) with an intercept on the same series: the line to read the two
                     above against (the compiled, speculating css-cgd kernel; no regression in front of it)
The three alternate in one process after a warm-up launch of each, every launch timed with a HIP event pair on the
caller's stream; medians and spreads (max - min) are reported with series per second, the status counts and the
evaluation counts (the fits are data dependent: a wave of the ARIMAX kernel runs as long as its slowest lane).
Prints one JSON line and writes it to --out.
--budget-s S (default 0 = none): no further round of launches is started once S seconds have passed since the first
launch, after at least one timed round; `launches_each` says how many were timed.
usage: python tools/bench_arimax.py [--series N] [--launches K] [--budget-s S] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-timeseries_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=1 << 16)
    ap.add_argument("--launches", type=int, default=5, help="timed launches of each call")
    ap.add_argument("--budget-s", type=float, default=0.0, help="start no further round after this many seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arimax", "bench_arimax.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import sparkts_amd._lib as L
    from sparkts_amd import buildinfo
    eng = L.Engine.get(0)
    N, T, k, p, d, q, lag = a.series, 1024, 2, 1, 1, 1, 1
    Kp = eng.arimax_num_coef(k, p, q, lag, True)
    dev = torch.device("cuda:0")
    torch.manual_seed(20261021)
    f64 = dict(dtype=torch.float64, device=dev)
    # x = 0.3 random walk + noise; y = 1.5 x0 - 0.7 x1 + an integrated ARMA(1, 1) with phi = 0.5, theta = 0.3
    x = (0.3 * torch.randn((N, k, T), **f64).cumsum(2) + torch.randn((N, k, T), **f64)).contiguous()
    e = torch.randn((N, T + 1), **f64)
    u = torch.empty((N, T), **f64)
    prev = torch.zeros(N, **f64)
    for t in range(T):
        prev = 0.5 * prev + e[:, t + 1] + 0.3 * e[:, t]
        u[:, t] = prev
    y = (u.cumsum(1) + 1.5 * x[:, 0] - 0.7 * x[:, 1]).contiguous()
    ys = (u.cumsum(1) + 1.5 * x[0, 0] - 0.7 * x[0, 1]).contiguous()       # the series that go with the shared matrix
    i32 = dict(dtype=torch.int32, device=dev)
    outs = {name: dict(coef=torch.empty((N, kk), **f64), ll=torch.empty(N, **f64), status=torch.empty(N, **i32),
                       n_eval=torch.empty(N, **i32), n_grad=torch.empty(N, **i32))
            for name, kk in (("arimax_shared", Kp), ("arimax_per_series", Kp), ("arima", 1 + p + q))}
    ts = torch.cuda.Stream()
    stream = ts.cuda_stream
    assert stream, "need a non-default stream"
    torch.cuda.synchronize()                                     # the engine's stream does not wait for torch's

    def arimax(name, rows, xs):
        o = outs[name]
        return lambda: eng.arimax_fit_device(rows.data_ptr(), N, T, T, x.data_ptr(), xs, k, p, d, q, lag, True, True,
                                             o["coef"].data_ptr(), o["ll"].data_ptr(), o["status"].data_ptr(),
                                             o["n_eval"].data_ptr(), o["n_grad"].data_ptr(), stream=stream,
                                             blocking=False)

    o = outs["arima"]
    calls = {
        "arimax_shared": arimax("arimax_shared", ys, 0),
        "arimax_per_series": arimax("arimax_per_series", y, k * T),
        "arima": lambda: eng.fit_batch_device(y.data_ptr(), N, T, T, p, d, q, True, o["coef"].data_ptr(),
                                              o["ll"].data_ptr(), o["status"].data_ptr(), o["n_eval"].data_ptr(),
                                              o["n_grad"].data_ptr(), stream=stream, blocking=False),
    }
    ms = {name: [] for name in calls}
    t0 = time.perf_counter()
    for i in range(1 + max(a.launches, 1)):                      # launch 0 of each is the warm-up
        if i >= 2 and a.budget_s > 0 and time.perf_counter() - t0 > a.budget_s:
            break
        for name, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            f()
            e1.record(ts)
            eng.synchronize()
            torch.cuda.synchronize()
            if i:
                ms[name].append(e0.elapsed_time(e1))
            print(json.dumps({"progress": name, "launch": i, "ms": e0.elapsed_time(e1)}), file=sys.stderr, flush=True)
    out = {"gpu": torch.cuda.get_device_name(0), "series": N, "T": T, "order": [p, d, q], "n_xcols": k,
           "xreg_max_lag": lag, "num_coef": Kp, "launches_each": len(ms["arima"]), "smear": eng.get_option("smear"),
           "library_sha": buildinfo.library_sha(), "source_sha": buildinfo.source_sha()}
    for name, v in ms.items():
        v = np.array(v)
        med = float(np.median(v)) * 1e-3
        st, ne = outs[name]["status"].cpu().numpy(), outs[name]["n_eval"].cpu().numpy()
        out[name] = {"median_ms": med * 1e3, "min_ms": float(v.min()), "max_ms": float(v.max()),
                     "spread_ms": float(v.max() - v.min()), "series_per_s": N / med,
                     "status_counts": {str(c): int(n) for c, n in zip(*np.unique(st, return_counts=True))},
                     "mean_n_eval": float(ne.mean()), "max_n_eval": int(ne.max()),
                     "mean_n_grad": float(outs[name]["n_grad"].cpu().numpy().mean())}
    out["arimax_per_series_over_arima"] = out["arimax_per_series"]["median_ms"] / out["arima"]["median_ms"]
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
