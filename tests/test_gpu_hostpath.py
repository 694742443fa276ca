"""The host fit path (arima_fit_batch: chunks of host_chunk series rotating over host_pipeline fit contexts, the tail
schedule, pinned result staging, the staged-upload ring) away from its defaults. Every case holds status, n_eval,
n_grad, coef, ll and flags to bit equality (NaNs included) against the oracle (the CPU restatement) and, where the batch
is too large for it, against arima_fit_batch_device on the same rows in one call plus the oracle on a sample of at most
512 rows that holds the first and last 16 rows of every planned chunk. The counters of arima_get_last_stats must sum
over the chunks. The chunk schedule itself is swept on the CPU by tests/test_hostplan_sim.py."""
import contextlib
import ctypes

import numpy as np
import pytest

import oracle as O
from test_gpu_parity import _device_sample, _same, check_fit

pytestmark = pytest.mark.gpu

HOST_OPTIONS = ("host_chunk", "host_pipeline", "host_tail", "host_copy_threads")
TAIL_MIN = 16384
C1 = (1, 0, 1, 1, [3.5, 0.3, 0.7])                      # ARIMA(1,0,1)+c and the sampler's base coefficients
C2 = (2, 1, 2, 1, [8.2, 0.2, 0.5, 0.3, 0.1])            # ARIMA(2,1,2)+c
KEYS = ("status", "n_eval", "n_grad", "coef", "ll", "flags")


@contextlib.contextmanager
def host_options(engine, **opts):
    prev = {o: engine.get_option(o) for o in HOST_OPTIONS}
    try:
        for o, v in opts.items():
            assert o in HOST_OPTIONS
            engine.set_option(o, v)
        yield prev
    finally:
        for o, v in prev.items():
            engine.set_option(o, v)


def plan(N, host_chunk, host_tail):
    """The host path's chunk boundaries, restated (host_plan.hpp host_chunk_starts)."""
    chunk = min(host_chunk, N)
    starts, f = [], 0
    while f < N:
        starts.append(f)
        rem = N - f
        n = min(chunk, rem)
        if host_tail and rem <= 2 * chunk and rem > TAIL_MIN:
            n = min(chunk, max(TAIL_MIN, (rem + 1) // 2))
        f += n
    return starts + [N]


def sizes(starts):
    return [b - a for a, b in zip(starts[:-1], starts[1:])]


def sample_rows(N, plans, extra=()):
    """At most 512 rows: the first and last 16 of every chunk of every plan, `extra`, and random rows up to 512."""
    rows = set(int(r) for r in extra)
    for starts in plans:
        for a, b in zip(starts[:-1], starts[1:]):
            rows.update(range(a, min(a + 16, b)))
            rows.update(range(max(b - 16, a), b))
    assert len(rows) <= 512
    for r in np.random.default_rng(N).permutation(N):
        if len(rows) >= min(512, N):
            break
        rows.add(int(r))
    return np.array(sorted(rows))


def oracle_fit(rows, p, d, q, I, method=0, user_init=None):
    st, coef, ll, cnt = O.fit_batch(rows, p, d, q, I, method, user_init)
    flags = np.array([O.model_flags(coef[i], p, q, I) if st[i] == 0 else 0 for i in range(len(st))], dtype=np.uint8)
    return dict(status=st, coef=coef, ll=ll, n_eval=cnt[:, 0], n_grad=cnt[:, 1], flags=flags)


def take(res, rows):
    return {key: res[key][rows] for key in KEYS}


def identical(res, ref, ctx):
    for key in ("status", "n_eval", "n_grad", "flags"):
        assert np.array_equal(res[key], ref[key]), f"{ctx}: {key} differs at rows {np.nonzero(res[key] != ref[key])[0][:8]}"
    for key in ("coef", "ll"):
        assert res[key].shape == ref[key].shape, f"{ctx}: {key} shape"
        assert _same(res[key], ref[key]), f"{ctx}: {key} not bit-identical"


def device_fit(engine, dev, p, d, q, I, method=0, user_init=None):
    """arima_fit_batch_device on the rows in one call."""
    import torch
    N, T = dev.shape
    k = p + q + I
    r = [torch.empty((N, max(k, 1)), dtype=torch.float64, device=dev.device),
         torch.empty(N, dtype=torch.float64, device=dev.device)] + \
        [torch.empty(N, dtype=torch.int32, device=dev.device) for _ in range(3)] + \
        [torch.empty(N, dtype=torch.uint8, device=dev.device)]
    ui = None if user_init is None else torch.from_numpy(np.ascontiguousarray(user_init)).to(dev.device)
    engine.fit_batch_device(dev.data_ptr(), N, T, T, p, d, q, I, *[t.data_ptr() for t in r],
                            d_user_init=None if ui is None else ui.data_ptr(), method=method)
    o = [t.cpu().numpy() for t in r]
    return dict(coef=o[0][:, :k], ll=o[1], status=o[2], n_eval=o[3], n_grad=o[4], flags=o[5])


def host_fit(engine, rows, p, d, q, I, method=0, user_init=None, ctx="", **opts):
    """arima_fit_batch under the given host options; the call's stats must count every series and evaluation once."""
    with host_options(engine, **opts):
        res = engine.fit_batch(rows, p, d, q, bool(I), method, user_init)
        st = engine.stats()
    N = rows.shape[0]
    assert st["n_series"] == N, f"{ctx} {opts}: stats count {st['n_series']} series of {N}"
    assert st["n_eval"] == int(res["n_eval"].sum(dtype=np.int64)), f"{ctx} {opts}: stats n_eval {st['n_eval']}"
    assert st["n_grad"] == int(res["n_grad"].sum(dtype=np.int64)), f"{ctx} {opts}: stats n_grad {st['n_grad']}"
    return res


_cache = {}


def sampled(engine, N, T, model, seed):
    """Rows of the device sampler (device tensor and host copy), drawn once per shape."""
    key = (N, T, model[:4], seed)
    if key not in _cache:
        p, d, q, I, base = model
        dev = _device_sample(engine, N, T, p, d, q, I, base, 0.05, seed)
        _cache[key] = (dev, dev.cpu().numpy())
    return _cache[key]


# ---- 1. tail chunks never exceed host_chunk ----------------------------------------------------------------------
@pytest.mark.parametrize("N,host_chunk", [(20000, 10000), (16385, 9000), (40000, 16383)])
def test_tail_chunk_stays_within_host_chunk(engine, N, host_chunk):
    # 8193 <= host_chunk <= 16383 with more than 16384 series left: the tail schedule's 16384-series floor must not
    # lift a chunk above host_chunk (every per-context buffer is sized for the plan's largest chunk). Small rows: only
    # the row count reaches the schedule.
    import torch
    p, d, q, I, base = C1
    T = 48
    dev = _device_sample(engine, N, T, p, d, q, I, base, 0.05, 20261019)
    rows = dev.cpu().numpy()
    plans = [plan(N, host_chunk, 1), plan(N, host_chunk, 0)]
    assert max(sizes(plans[0])) <= host_chunk and plans[0] == plans[1]
    ref = device_fit(engine, dev, p, d, q, I)
    on = host_fit(engine, rows, p, d, q, I, ctx="tail", host_chunk=host_chunk, host_pipeline=3, host_tail=1)
    off = host_fit(engine, rows, p, d, q, I, ctx="flat", host_chunk=host_chunk, host_pipeline=3, host_tail=0)
    identical(on, off, "host_tail 1 vs 0")
    identical(on, ref, "host path vs device path")
    idx = sample_rows(N, plans)
    exp = oracle_fit(rows[idx], p, d, q, I)
    check_fit(take(on, idx), exp, f"tail ({N}, {host_chunk}) vs oracle")
    # the handle's buffers after the small chunks: a fit at the restored options regrows them and still matches
    again = host_fit(engine, rows, p, d, q, I, ctx="restored")
    identical(again, ref, "restored options vs device path")
    del dev
    torch.cuda.empty_cache()


# ---- 2. the tail schedule where it applies -------------------------------------------------------------------------
def test_tail_schedule_engaged(engine):
    import torch
    p, d, q, I, base = C1
    N, T, host_chunk = 70000, 48, 20000
    starts = plan(N, host_chunk, 1)
    assert sizes(starts) == [20000, 20000, 16384, 13616]
    dev = _device_sample(engine, N, T, p, d, q, I, base, 0.05, 20261020)
    rows = dev.cpu().numpy()
    ref = device_fit(engine, dev, p, d, q, I)
    idx = sample_rows(N, [starts, plan(N, host_chunk, 0)])
    exp = oracle_fit(rows[idx], p, d, q, I)
    for pipeline in (1, 3):
        res = host_fit(engine, rows, p, d, q, I, ctx="tail engaged", host_chunk=host_chunk, host_pipeline=pipeline,
                       host_tail=1)
        identical(res, ref, f"host_pipeline={pipeline} vs device path")
        check_fit(take(res, idx), exp, f"host_pipeline={pipeline} vs oracle")
    del dev
    torch.cuda.empty_cache()


# ---- 3. chunk boundaries, pipelines longer than the call ---------------------------------------------------------
def _c2_T100(engine):
    if "c2_T100" not in _cache:
        p, d, q, I, _ = C2
        _, rows = sampled(engine, 129, 100, C2, 4711)
        _cache["c2_T100"] = (rows, oracle_fit(rows, p, d, q, I))
    return _cache["c2_T100"]


@pytest.mark.parametrize("N", [63, 64, 65, 127, 128, 129])
def test_chunk_boundaries(engine, N):
    p, d, q, I, _ = C2
    rows, exp = _c2_T100(engine)
    rows, exp = rows[:N], take(exp, slice(0, N))
    for pipeline in (1, 2, 6):                       # 6: more contexts than chunks
        res = host_fit(engine, rows, p, d, q, I, ctx=f"N={N}", host_chunk=64, host_pipeline=pipeline)
        check_fit(res, exp, f"N={N} host_pipeline={pipeline}")
    # grow (one large chunk), then the small chunks again on buffers that need no regrowing
    for host_chunk in (1 << 18, 64):
        res = host_fit(engine, rows, p, d, q, I, ctx=f"N={N}", host_chunk=host_chunk, host_pipeline=2)
        check_fit(res, exp, f"N={N} host_chunk={host_chunk} after the sweep")


# ---- 4. per-series user inits across chunks ------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1])
def test_user_init_across_chunks(engine, method):
    p, d, q, I, base = C2
    N, T, k = 200, 100, 5
    _, rows = sampled(engine, N, T, C2, 1234)
    ui = np.asarray(base)[None, :] + np.random.default_rng(5).uniform(-0.1, 0.1, (N, k))   # a different row per series
    ui[70] = [np.nan, np.inf, -np.inf, np.nan, 0.25]                                       # inside the second chunk
    exp = oracle_fit(rows, p, d, q, I, method, ui)
    res = host_fit(engine, rows, p, d, q, I, method, ui, ctx=f"user_init method={method}", host_chunk=64)
    check_fit(res, exp, f"user_init method={method}")
    one = host_fit(engine, rows, p, d, q, I, method, ui, ctx="user_init one chunk")
    identical(res, one, "chunked vs one chunk")


# ---- 5. models that end in a shortcut or a uniform status, through chunks -----------------------------------------
SHORTCUTS = {
    "zero_width": ((0, 1, 0, 0), 100, 0),            # k = 0: coef has no columns
    "ar_only": ((2, 0, 0, 1), 100, 0),               # the AR-only shortcut
    "too_short": ((2, 1, 2, 1), 6, 0),               # every series fails alike
    "unsupported_method": ((1, 0, 1, 1), 100, 99),
}


@pytest.mark.parametrize("name", sorted(SHORTCUTS))
def test_shortcut_models_through_chunks(engine, name):
    (p, d, q, I), T, method = SHORTCUTS[name]
    N = 130
    _, rows = sampled(engine, N, T, C2, 99)
    exp = oracle_fit(rows, p, d, q, I, method)
    one = host_fit(engine, rows, p, d, q, I, method, ctx=f"{name} one chunk")
    res = host_fit(engine, rows, p, d, q, I, method, ctx=f"{name} chunked", host_chunk=64)
    assert res["coef"].shape == (N, p + q + I)
    identical(res, one, f"{name}: chunked vs one chunk")
    check_fit(res, exp, name)
    if name in ("too_short", "unsupported_method"):
        assert np.all(res["status"] == res["status"][0]) and res["status"][0] != 0


# ---- 6. optional outputs left out ----------------------------------------------------------------------------------
SENT = -12345.0


@pytest.mark.parametrize("absent", [("n_eval",), ("n_grad",), ("flags",), ("n_eval", "n_grad", "flags")])
def test_null_optional_outputs(engine, absent):
    p, d, q, I, _ = C2
    N, T, k, pad = 130, 100, 5, 64
    _, rows = sampled(engine, N, T, C2, 99)
    # the reference: every output present, itself held to the oracle
    full = host_fit(engine, rows, p, d, q, I, ctx="all outputs", host_chunk=64)
    check_fit(full, oracle_fit(rows, p, d, q, I), "all outputs")
    out = dict(coef=np.full(N * k + pad, SENT), ll=np.full(N + pad, SENT), status=np.full(N + pad, -77, np.int32),
               n_eval=np.full(N + pad, -77, np.int32), n_grad=np.full(N + pad, -77, np.int32),
               flags=np.full(N + pad, 0xEE, np.uint8))
    ctype = dict(coef=ctypes.c_double, ll=ctypes.c_double, status=ctypes.c_int32, n_eval=ctypes.c_int32,
                 n_grad=ctypes.c_int32, flags=ctypes.c_uint8)

    def arg(key):
        return None if key in absent else out[key].ctypes.data_as(ctypes.POINTER(ctype[key]))

    with host_options(engine, host_chunk=64):
        rc = engine.L.arima_fit_batch(engine.h, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), N, T, p, d, q, I,
                                      0, None, arg("coef"), arg("ll"), arg("status"), arg("n_eval"), arg("n_grad"),
                                      arg("flags"))
        st = engine.stats()
    assert rc == 0
    for key in KEYS:
        n = N * k if key == "coef" else N
        tail = out[key][n:]
        assert np.all(tail == tail[0]) and tail[0] in (SENT, -77, 0xEE), f"{key}: written past its end"
        if key in absent:
            assert np.all(out[key] == out[key][0]), f"{key}: a NULL output was written somewhere"
            continue
        got = out[key][:n].reshape(full[key].shape)
        assert _same(got, full[key]) if key in ("coef", "ll") else np.array_equal(got, full[key]), key
    assert st["n_series"] == N and st["n_eval"] == int(full["n_eval"].sum()) and st["n_grad"] == int(full["n_grad"].sum())


# ---- 7. uploads through the pinned ring (host_copy_threads > 0) --------------------------------------------------
def _c2_T1024(engine):
    if "c2_T1024" not in _cache:
        p, d, q, I, _ = C2
        dev, rows = sampled(engine, 2048, 1024, C2, 777)
        _cache["c2_T1024"] = (dev, rows, oracle_fit(rows, p, d, q, I))
    return _cache["c2_T1024"]


def test_staged_uploads_ring_reused(engine):
    # 7 chunks of 300 x 1024 through the 3-block ring: every block is refilled under its event; every series vs oracle
    p, d, q, I, _ = C2
    _, rows, exp = _c2_T1024(engine)
    assert len(sizes(plan(2048, 300, 1))) == 7
    base = host_fit(engine, rows, p, d, q, I, ctx="ring", host_chunk=300, host_pipeline=3, host_copy_threads=0)
    check_fit(base, exp, "host_copy_threads=0")
    for threads in (1, 4):
        res = host_fit(engine, rows, p, d, q, I, ctx="ring", host_chunk=300, host_pipeline=3, host_copy_threads=threads)
        identical(res, base, f"host_copy_threads={threads} vs 0")


def test_staged_uploads_split_copy(engine):
    # one chunk of 2048 x 1024 = 16 MiB: four threads copy 4 MiB parts of one block
    p, d, q, I, _ = C2
    dev, rows, exp = _c2_T1024(engine)
    assert engine.get_option("host_chunk") >= 2048
    ref = device_fit(engine, dev, p, d, q, I)
    idx = sample_rows(2048, [plan(2048, engine.get_option("host_chunk"), 1)])
    base = host_fit(engine, rows, p, d, q, I, ctx="split", host_copy_threads=0)
    for threads in (1, 4):
        res = host_fit(engine, rows, p, d, q, I, ctx="split", host_copy_threads=threads)
        identical(res, base, f"host_copy_threads={threads} vs 0")
        identical(res, ref, f"host_copy_threads={threads} vs device path")
        check_fit(take(res, idx), take(exp, idx), f"host_copy_threads={threads} vs oracle")


def test_staged_uploads_across_blocks(engine):
    # 17000 x 1000 doubles = 136 MB in one chunk: more than one 128 MiB block, the block boundary inside row 16777
    import torch
    p, d, q, I, base_coef = C1
    N, T = 17000, 1000
    assert engine.get_option("host_chunk") >= N
    edge = (128 << 20) // (T * 8)
    assert (128 << 20) % (T * 8) != 0 and edge == 16777
    dev = _device_sample(engine, N, T, p, d, q, I, base_coef, 0.05, 31337)
    rows = dev.cpu().numpy()
    ref = device_fit(engine, dev, p, d, q, I)
    del dev
    torch.cuda.empty_cache()
    idx = sample_rows(N, [plan(N, engine.get_option("host_chunk"), 1)], extra=range(edge - 8, edge + 8))
    exp = oracle_fit(rows[idx], p, d, q, I)
    base = host_fit(engine, rows, p, d, q, I, ctx="blocks", host_copy_threads=0)
    for threads in (1, 4):
        res = host_fit(engine, rows, p, d, q, I, ctx="blocks", host_copy_threads=threads)
        identical(res, base, f"host_copy_threads={threads} vs 0")
        identical(res, ref, f"host_copy_threads={threads} vs device path")
        check_fit(take(res, idx), exp, f"host_copy_threads={threads} vs oracle")
