"""The gradient pass the fit kernels no longer run: after a line search the optimizer's next top-of-iteration test --
convergence on objective values, MaxIter, MaxEval -- is known before the gradient at the new point is, and when it is
going to stop the fit nothing reads that gradient (cg_lane.hpp, PC_LS_DONE). The request is then not posted; it is
still counted in n_grad as the reference counts it, and in the stats' skipped_g. Here: the bulk path (two waves and
a tail; ten waves of short rows), the runtime-order path, the express path and the forced drain merge -- all six
outputs bit-identical to the CPU restatement, gradient passes + skipped_g == the sum of n_grad, and skipped_g == the
converged fits (each ran a line search: the first top-of-iteration test has no previous value to converge on). The rows
come from seeds at which every fit converges: a fit whose point turns non-finite counts gradients without a pass as
well (the NaN gradient, the NaN fast-forward), which the identity does not cover -- before this change either. Fits
that fail are compared with the restatement in tests/test_gpu_parity.py. The CPU side is tests/test_skipg_sim.py."""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

C2_BASE = [8.2, 0.2, 0.5, 0.3, 0.1]
GEN_BASE = [0.5, 0.3, -0.2, 0.1, 0.05, -0.05, 0.1, 0.2]
# (p, d, q, I, N, T, model of the rows, seed, options)
CASES = {
    "bulk_212": (2, 1, 2, 1, 130, 64, C2_BASE, 1, {}),
    "bulk_101": (1, 0, 1, 1, 1025, 16, [1.0, 0.4, 0.3], 2, {}),
    "runtime_order_601": (6, 0, 1, 1, 70, 48, GEN_BASE, 1, {}),
    "express_212": (2, 1, 2, 1, 130, 64, C2_BASE, 1, {"express_blocks": 4}),
    "merge_212": (2, 1, 2, 1, 130, 64, C2_BASE, 1, {"merge_live": 64}),
}
_ROWS = {}


def _rows_and_oracle(p, d, q, I, N, T, base, seed):
    """Rows of the model (standard normal noise through addTimeDependentEffects) on the device, and the
    restatement's fit of them, once per shape."""
    import torch
    key = (p, d, q, I, N, T, seed)
    if key not in _ROWS:
        rng = np.random.default_rng(seed)
        host = np.stack([O.add_time_dependent_effects(rng.standard_normal(T), p, d, q, I, base) for _ in range(N)])
        buf = torch.as_tensor(host, device="cuda")
        st, coef, ll, cnt = O.fit_batch(host, p, d, q, I)
        flags = np.array([O.model_flags(coef[i], p, q, I) if st[i] == 0 else 0 for i in range(N)], dtype=np.uint8)
        _ROWS[key] = (buf, dict(status=st, coef=coef, ll=ll, n_eval=cnt[:, 0], n_grad=cnt[:, 1], flags=flags))
    return _ROWS[key]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("name", list(CASES))
def test_dead_gradient_is_skipped_and_counted(engine, name):
    import torch
    p, d, q, I, N, T, base, seed, options = CASES[name]
    k = p + q + I
    rows, exp = _rows_and_oracle(p, d, q, I, N, T, base, seed)
    dev = rows.device
    out = dict(coef=torch.full((N, k), -7.25, dtype=torch.float64, device=dev),
               ll=torch.empty(N, dtype=torch.float64, device=dev),
               status=torch.empty(N, dtype=torch.int32, device=dev),
               n_eval=torch.empty(N, dtype=torch.int32, device=dev),
               n_grad=torch.empty(N, dtype=torch.int32, device=dev),
               flags=torch.empty(N, dtype=torch.uint8, device=dev))
    prev = {opt: engine.get_option(opt) for opt in options}
    try:
        for opt, v in options.items():
            engine.set_option(opt, v)
        engine.fit_batch_device(rows.data_ptr(), N, T, T, p, d, q, I, out["coef"].data_ptr(), out["ll"].data_ptr(),
                                out["status"].data_ptr(), out["n_eval"].data_ptr(), out["n_grad"].data_ptr(),
                                out["flags"].data_ptr())
        st = engine.stats()
    finally:
        for opt, v in prev.items():
            engine.set_option(opt, v)
    res = {key: v.cpu().numpy() for key, v in out.items()}
    print(name, {f: st[f] for f in ("g_passes", "ride_passes", "express_g_passes", "skipped_g", "n_grad", "n_eval",
                                   "express_series", "merge_series", "express_blocks")})
    # the six outputs against the restatement (failed fits: NaN coefficients and LL, flags 0)
    ok = exp["status"] == 0
    assert ok.all()                                     # the seeds' property (module docstring)
    assert np.array_equal(res["status"], exp["status"])
    assert np.array_equal(res["n_eval"], exp["n_eval"]) and np.array_equal(res["n_grad"], exp["n_grad"])
    assert _bits_equal(res["coef"][ok], exp["coef"][ok]) and np.all(np.isnan(res["coef"][~ok]))
    assert _bits_equal(res["ll"][ok], exp["ll"][ok]) and np.all(np.isnan(res["ll"][~ok]))
    assert np.array_equal(res["flags"], exp["flags"])
    if "express_blocks" in options:                     # series finish on express waves, whose skips are summed too
        assert st["express_blocks"] == options["express_blocks"]
        assert st["express_series"] > 0 and st["express_g_passes"] > 0, st
    if "merge_live" in options:                         # lanes move between waves with their state
        assert st["merge_series"] > 0, st
    assert st["fault"] == 0 and st["series_done"] == st["n_series"] == N
    # every gradient the reference counts either ran a pass or was skipped
    n_grad = int(exp["n_grad"].sum(dtype=np.int64))
    assert st["n_grad"] == n_grad > 0
    assert st["g_passes"] - st["ride_passes"] + st["express_g_passes"] + st["skipped_g"] == n_grad, st
    # one skip per converged fit that ran a line search
    assert st["skipped_g"] == int((ok & (exp["n_grad"] >= 2)).sum()) > 0, st
    assert engine.stats() == st
