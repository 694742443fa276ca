"""Measure the design-matrix regressions on one GPU (device-resident, f64) at N x 1024:

  arx_shared      arima_arx_fit_batch_device, ARX(2, 1, includeOriginalX), 2 regressor columns shared by every series
  arx_per_series  the same with one regressor matrix per series
  bgtest          arima_bgtest_batch_device, max_lag 4, one factor column per series
  co_shared       arima_regarima_co_fit_batch_device (Cochrane-Orcutt, max_iter 10), the 2 regressor columns shared
  co_per_series   the same with one regressor matrix per series
The five alternate in one process after a warm-up launch of each, every launch timed with a HIP event pair on the
caller's stream; medians and spreads (max - min) are reported, with series per second and the achieved bytes per second
against the traffic model of DESIGN.md 5.7 (2 C^2 R 8 bytes per series for the QR; the tests add their second assembly
and the calculateRSquared pass). For context only, oracle.ols (the C restatement of the same QR) over the designs of
the first --cpu-series series on --cpu-threads host threads. The Cochrane-Orcutt legs run a data-dependent number of
QRs per series (n_iter + 1): they report the histogram of n_iter and its mean next to series per second,
and no traffic model. Prints one JSON line and writes it to --out.
usage: python tools/bench_regress.py [--series N] [--launches K] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-timeseries_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def model_bytes(C, R, test):
    """Bytes per series of the 5.7 traffic model: the assembly writes (C + 1) R doubles, the QR moves about 2 C^2 R;
    a test assembles again and reads the design once more."""
    return 8 * ((C + 1) * R + 2 * C * C * R + (2 * (C + 1) * R if test else 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=1 << 16)
    ap.add_argument("--launches", type=int, default=5, help="timed launches of each call (at least 5)")
    ap.add_argument("--cpu-series", type=int, default=2048)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regress", "bench_regress.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import oracle as O
    import sparkts_amd._lib as L
    from sparkts_amd import buildinfo
    eng = L.Engine.get(0)
    N, T, k = a.series, 1024, 2
    dev = torch.device("cuda:0")
    torch.manual_seed(20261020)
    f64 = dict(dtype=torch.float64, device=dev)
    x = torch.randn((N, k, T), **f64)                            # per series k rows of T values
    y = (torch.randn((N, T), **f64).cumsum(1) * 0.1 + x.sum(1) + 2.0).contiguous()
    coef = [torch.empty((N, 7), **f64) for _ in range(2)]
    stat, pv = torch.empty(N, **f64), torch.empty(N, **f64)
    st = [torch.empty(N, dtype=torch.int32, device=dev) for _ in range(5)]
    co = [(torch.empty((N, 1 + k), **f64), torch.empty(N, **f64), torch.empty(N, dtype=torch.int32, device=dev))
          for _ in range(2)]
    ts = torch.cuda.Stream()
    stream = ts.cuda_stream
    assert stream, "need a non-default stream"
    torch.cuda.synchronize()                                     # the engine's stream does not wait for torch's
    calls = {
        "arx_shared": lambda: eng.arx_fit_device(y.data_ptr(), N, T, T, x.data_ptr(), 0, k, 2, 1, True, False,
                                                 coef[0].data_ptr(), st[0].data_ptr(), stream=stream, blocking=False),
        "arx_per_series": lambda: eng.arx_fit_device(y.data_ptr(), N, T, T, x.data_ptr(), k * T, k, 2, 1, True, False,
                                                     coef[1].data_ptr(), st[1].data_ptr(), stream=stream,
                                                     blocking=False),
        "bgtest": lambda: eng.bgtest_device(y.data_ptr(), N, T, T, x.data_ptr(), k * T, 1, 4, stat.data_ptr(),
                                            pv.data_ptr(), st[2].data_ptr(), stream=stream, blocking=False),
        "co_shared": lambda: eng.regarima_co_fit_device(y.data_ptr(), N, T, T, x.data_ptr(), 0, k, 10,
                                                        co[0][0].data_ptr(), co[0][1].data_ptr(), co[0][2].data_ptr(),
                                                        st[3].data_ptr(), stream=stream, blocking=False),
        "co_per_series": lambda: eng.regarima_co_fit_device(y.data_ptr(), N, T, T, x.data_ptr(), k * T, k, 10,
                                                            co[1][0].data_ptr(), co[1][1].data_ptr(),
                                                            co[1][2].data_ptr(), st[4].data_ptr(), stream=stream,
                                                            blocking=False),
    }
    shape = {"arx_shared": (7, T - 2, False), "arx_per_series": (7, T - 2, False), "bgtest": (6, T - 4, True)}
    ms = {name: [] for name in calls}
    for i in range(1 + max(a.launches, 5)):                      # launch 0 of each is the warm-up
        for name, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            f()
            e1.record(ts)
            torch.cuda.synchronize()
            if i:
                ms[name].append(e0.elapsed_time(e1))
            print(json.dumps({"progress": name, "launch": i, "ms": e0.elapsed_time(e1)}), file=sys.stderr, flush=True)
    out = {"gpu": torch.cuda.get_device_name(0), "series": N, "T": T, "launches_each": len(ms["bgtest"]),
           "library_sha": buildinfo.library_sha(), "source_sha": buildinfo.source_sha()}
    for name, v in ms.items():
        v = np.array(v)
        med = float(np.median(v)) * 1e-3
        out[name] = {"median_ms": med * 1e3, "min_ms": float(v.min()), "max_ms": float(v.max()),
                     "spread_ms": float(v.max() - v.min()), "series_per_s": N / med}
        if name in shape:
            C, R, test = shape[name]
            out[name].update({"columns": C, "rows": R, "model_bytes_per_series": model_bytes(C, R, test),
                              "model_bytes_per_s": N * model_bytes(C, R, test) / med})
    for name, (_, _, n_iter) in zip(("co_shared", "co_per_series"), co):
        it = n_iter.cpu().numpy()
        out[name].update({"columns": 1 + k, "rows": T, "max_iter": 10, "mean_n_iter": float(it.mean()),
                          "n_iter_histogram": {str(c): int(n) for c, n in zip(*np.unique(it, return_counts=True))}})
    for name, s in zip(calls, st):
        s = s.cpu().numpy()
        out[name]["status_counts"] = {str(c): int(n) for c, n in zip(*np.unique(s, return_counts=True))}

    # context: the C restatement of the same QR on the host, the ARX designs of the first series
    n = min(a.cpu_series, N)
    yh, xh = y[:n].cpu().numpy(), x[:n].cpu().numpy()
    designs = [np.stack([yh[i, 1:T - 1], yh[i, 0:T - 2], xh[i, 0, 1:T - 1], xh[i, 1, 1:T - 1], xh[i, 0, 2:],
                         xh[i, 1, 2:]], axis=1) for i in range(n)]
    O.ols(yh[0, 2:], designs[0], True)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(a.cpu_threads) as pool:
        res = list(pool.map(lambda i: O.ols(yh[i, 2:], designs[i], True), range(n)))
    dt = time.perf_counter() - t0
    got = coef[1][:n].cpu().numpy()
    out["cpu_oracle_ols"] = {"series": n, "threads": a.cpu_threads, "seconds": dt, "series_per_s": n / dt,
                             "identical_to_device": bool(all(r[0] == 0 and np.array_equal(r[1], got[i])
                                                             for i, r in enumerate(res)))}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
