"""The three promises include/sparkts_arima.h makes about streams and threads, pinned from the caller's side.

1. Every `*_device` entry point runs on the caller's hipStream_t: it is ordered behind the caller's earlier work on that
   stream and everything it forks internally is joined back before the call's end on that stream.
2. Calls on one handle are ordered on the device whichever streams they use (fits under fit_pipeline > 1 run concurrently
   unless their buffers meet); arima_synchronize and both stats getters wait for the last call's device work.
3. Calls on one handle are serialised internally, so one handle may be driven from several host threads.

Mis-ordering shows only while the producer is still running, so every scenario first puts a delay (ordinary torch work,
timed once per session: at least 20 ms, host-side enqueue of the few calls that follow costs well under 1 ms) on the
producing stream. A control per stream pair proves the detector without the library: a buffer of decoys is overwritten
behind the delay on one stream and read from the other with no wait (the read must see the decoy) and with wait_stream
(it must see the real data). A scenario whose control failed fails with that message.

Inputs hold decoys (finite, valid values of another seed) until the real data is copied over them on the caller's stream;
outputs hold sentinels (-7.25, -77, 0xEE), are snapshot on the caller's stream straight after the call and compared after
that stream alone has been synchronised -- bit for bit against the CPU restatement the entry point's own test uses.
Padding columns (ld = T + 3, ld_out = T + 5) and 8 guard rows either side of every output must keep their sentinel.
Every wait is on work issued earlier from the host, so no schedule can deadlock.
"""
import contextlib
import math
import threading

import numpy as np
import pytest

import argarch_ref as AR
import oracle as O
import regress_ref as RR
import smallfit_ref as SR
import sparkts_amd._lib as L
from conftest import load_case
from test_gpu_autofit import check_autofit
from test_gpu_diag import _check as diag_check, _p_close, _ref as diag_ref
from test_gpu_hostpath import C1, C2, _c2_T100, device_fit, identical, oracle_fit, plan, sample_rows, sampled, take
from test_gpu_parity import _device_sample, _same, check_fit
from test_gpu_regress import _arx_case

pytestmark = pytest.mark.gpu

SENT, ISENT, BSENT = -7.25, -77, 0xEE
G = 8                                   # guard rows before and after every output
DELAY_TARGET_MS, DELAY_MIN_MS = 50.0, 20.0
DELAY_DOUBLES = 1 << 26                 # 512 MiB scaled in place per launch
OPTIONS = ("fit_pipeline", "search_lanes", "fit_slice_bytes", "diag_slice_bytes", "autofit_slice", "regress_slice_bytes")
JOIN_S = 120

_memo = {}


def memo(key, make):
    """References are computed once, shared among the tests and left unchanged."""
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


@contextlib.contextmanager
def options(engine, **opts):
    assert set(opts) <= set(OPTIONS)
    prev = {o: engine.get_option(o) for o in opts}
    try:
        for o, v in opts.items():
            engine.set_option(o, v)
        yield
    finally:
        for o, v in prev.items():
            engine.set_option(o, v)


def same(got, want, what):
    """Bit for bit with NaNs in the same places (floats), equal (integers)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.dtype.kind == "f":
        assert _same(got, want), f"{what}: not bit-identical at {np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5].tolist()}"
    else:
        assert np.array_equal(got, want), f"{what}: differs at {np.argwhere(got != want)[:5].tolist()}"


# ---- 0. the delay and its control -----------------------------------------------------------------------------------
class Rig:
    """Three caller streams, the delay and the control of every producer -> consumer pair the scenarios use."""

    PAIRS = ((0, 1), (1, 2), (2, 0))

    def __init__(self, engine):
        import torch
        self.torch = torch
        self.dev = torch.device(f"cuda:{engine.device}")
        self.streams = [torch.cuda.Stream(self.dev) for _ in range(3)]
        self.block = torch.ones(DELAY_DOUBLES, dtype=torch.float64, device=self.dev)
        torch.cuda.synchronize(self.dev)
        self._time(8)                                        # the first launches load the kernel and raise the clocks
        per = self._time(32) / 32.0
        self.reps = max(1, math.ceil(DELAY_TARGET_MS / max(per, 1e-3)))
        self.ms = self._time(self.reps)
        if not 0.6 * DELAY_TARGET_MS <= self.ms <= 2.0 * DELAY_TARGET_MS:
            self.reps = max(1, math.ceil(self.reps * DELAY_TARGET_MS / max(self.ms, 1e-3)))
            self.ms = self._time(self.reps)
        self.error = None
        if self.ms < DELAY_MIN_MS:
            self.error = f"the delay ran {self.ms:.1f} ms, below the {DELAY_MIN_MS} ms the scenarios need"
        self.control = {}
        for pair in self.PAIRS:
            self.control[pair] = self.error or self._control(*pair)
        print(f"\n[test_gpu_streams] delay {self.ms:.1f} ms ({self.reps} launches); controls {self.control}")

    def _spin(self, reps):
        for _ in range(reps):
            self.block.mul_(1.0)

    def _time(self, reps):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.streams[0]):
            a.record()
            self._spin(reps)
            b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def host(self, t, s):
        """A tensor's values, read through stream s (the copy is synchronous with s alone)."""
        with self.torch.cuda.stream(s):
            return t.cpu().numpy()

    def _control(self, i, j):
        torch = self.torch
        a, b = self.streams[i], self.streams[j]
        real = torch.from_numpy(np.random.default_rng(1).standard_normal((130, 100))).to(self.dev)
        decoy = torch.from_numpy(np.random.default_rng(2).standard_normal((130, 100))).to(self.dev)
        buf = decoy.clone()
        torch.cuda.synchronize(self.dev)
        with torch.cuda.stream(a):
            self._spin(self.reps)
            buf.copy_(real, non_blocking=True)
        with torch.cuda.stream(b):
            early = buf.clone()
        b.synchronize()
        early = self.host(early, b)
        a.synchronize()
        buf.copy_(decoy)
        torch.cuda.synchronize(self.dev)
        with torch.cuda.stream(a):
            self._spin(self.reps)
            buf.copy_(real, non_blocking=True)
        b.wait_stream(a)
        with torch.cuda.stream(b):
            late = buf.clone()
        b.synchronize()
        late = self.host(late, b)
        a.synchronize()
        if not np.array_equal(early, decoy.cpu().numpy()):
            return (f"control {i}->{j}: a read with no wait did not see the decoy, so a missing wait would pass unnoticed: "
                    f"the delay ({self.ms:.1f} ms) is too short, or the two streams share a hardware queue")
        if not np.array_equal(late, real.cpu().numpy()):
            return f"control {i}->{j}: a read after wait_stream did not see the real data"
        return None

    def delay(self):
        """The delay on the current stream. A scenario behind a delay that no control has proven fails, never passes."""
        bad = self.error or next((m for m in self.control.values() if m), None)
        if bad:
            pytest.fail(bad)
        self._spin(self.reps)

    def chain(self, *idx):
        """The streams of a scenario whose consecutive calls go producer -> consumer along idx; every pair's control must
        have seen the decoy."""
        for i, j in zip(idx[:-1], idx[1:]):
            if i != j and self.control[(i, j)]:
                pytest.fail(self.control[(i, j)])
        return [self.streams[i] for i in idx]


@pytest.fixture(scope="session")
def rig(engine):
    return Rig(engine)


def test_control_sees_the_decoy(rig):
    assert rig.error is None, rig.error
    assert rig.ms >= DELAY_MIN_MS
    for pair in Rig.PAIRS:
        assert rig.control[pair] is None, rig.control[pair]


class In:
    """A strided device input (N x cols, row stride ld): the padding holds the sentinel and the payload a decoy until
    load() copies the real values over it on the current stream."""

    def __init__(self, dev, real, decoy, ld=None):
        import torch
        real, decoy = np.ascontiguousarray(real, dtype=np.float64), np.ascontiguousarray(decoy, dtype=np.float64)
        if real.ndim == 1:
            real, decoy = real[:, None], decoy[:, None]
        assert real.shape == decoy.shape and np.all(np.isfinite(decoy))
        self.n, self.cols = real.shape
        self.ld = ld or self.cols
        self.full = torch.full((self.n, self.ld), SENT, dtype=torch.float64, device=dev)
        self.full[:, :self.cols] = torch.from_numpy(decoy).to(dev)
        self.real = torch.from_numpy(real).to(dev)
        self.want = real
        self.ptr = self.full.data_ptr()

    def load(self):
        self.full[:, :self.cols].copy_(self.real, non_blocking=True)

    def untouched(self, snap, what):
        """A snapshot taken after the call: the real rows, the padding still the sentinel."""
        same(snap[:, :self.cols], self.want, f"{what}: input changed")
        assert np.all(snap[:, self.cols:] == SENT), f"{what}: input padding written"


class Out:
    """A sentinel-filled device output of n rows (cols None: a vector) with G guard rows either side."""

    def __init__(self, dev, n, cols=None, dtype="float64", ld=None):
        import torch
        self.sent = {"float64": SENT, "int32": ISENT, "uint8": BSENT}[dtype]
        self.n, self.cols = n, cols
        self.ld = None if cols is None else (ld or cols)
        shape = (G + n + G,) if cols is None else (G + n + G, self.ld)
        self.full = torch.full(shape, self.sent, dtype=getattr(torch, dtype), device=dev)
        self.ptr = self.full[G:].data_ptr()

    def body(self, snap, what):
        """The payload of a snapshot; guards and padding must hold the sentinel."""
        assert np.all(snap[:G] == self.sent) and np.all(snap[G + self.n:] == self.sent), f"{what}: guard rows written"
        rows = snap[G:G + self.n]
        if self.cols is None:
            return rows
        assert np.all(rows[:, self.cols:] == self.sent), f"{what}: padding columns written"
        return rows[:, :self.cols]


def fit_outs(dev, N, k):
    return [Out(dev, N, k), Out(dev, N)] + [Out(dev, N, dtype="int32") for _ in range(3)] + [Out(dev, N, dtype="uint8")]


FIT_KEYS = ("coef", "ll", "status", "n_eval", "n_grad", "flags")
MODEL_KEYS = ("coef", "obj", "status", "n_eval", "n_grad")
DIAG_KEYS = L.Engine.DIAG_OUTPUTS


def model_outs(dev, N, K):
    return [Out(dev, N, K), Out(dev, N)] + [Out(dev, N, dtype="int32") for _ in range(3)]


def diag_outs(dev, N, max_lag):
    return [Out(dev, N, max_lag)] + [Out(dev, N) for _ in range(3)]


def ptrs(outs):
    return [o.ptr for o in outs]


def snapshots(tensors):
    """Clones on the current stream (allocated there too)."""
    return [t.full.clone() for t in tensors]


def bodies(rig, s, outs, snaps, what):
    return [o.body(rig.host(x, s), what) for o, x in zip(outs, snaps)]


class Scenario:
    """One row of section 1: inputs, outputs, the call (stream handle -> None), the check of the outputs' payloads, and
    an optional follow-up that runs after the options are restored."""

    def __init__(self, ins, outs, call, check, after=None):
        self.ins, self.outs, self.call, self.check, self.after = ins, outs, call, check, after


def run_scenario(rig, s, sc, what):
    torch = rig.torch
    torch.cuda.synchronize(rig.dev)                          # the buffers are set up before the stream is used
    with torch.cuda.stream(s):
        rig.delay()
        for i in sc.ins:
            i.load()
        sc.call(s.cuda_stream)
        snaps = snapshots(sc.outs)
        in_snaps = snapshots(sc.ins)
    s.synchronize()                                          # the caller's stream alone, never the handle
    got = bodies(rig, s, sc.outs, snaps, what)
    for i, x in zip(sc.ins, in_snaps):
        i.untouched(rig.host(x, s), what)
    return got


# ---- 1. every device entry point on a caller stream ---------------------------------------------------------------------
def _walks(seed, N, T):
    return np.random.default_rng(seed).standard_normal((N, T)).cumsum(axis=1) + 2.0


def _fit_rows(engine):
    """130 x 100 rows of the sampler stream test_gpu_hostpath._c2_T100 draws (its 129 and the next one), and decoys."""
    def make():
        first, _ = _c2_T100(engine)
        _, rows = sampled(engine, 130, 100, C2, 4711)
        assert np.array_equal(rows[:129], first)
        _, decoy = sampled(engine, 130, 100, C2, 4712)
        return rows, decoy
    return memo("fit_rows", make)


def _user_init(N, seed):
    return np.asarray(C2[4])[None, :] + np.random.default_rng(seed).uniform(-0.1, 0.1, (N, 5))


FIT_MODELS = {"cgd_user_init": ((2, 1, 2, 1), 0, True), "bobyqa_user_init": ((2, 1, 2, 1), 1, True),
              "ar_only": ((2, 0, 0, 1), 0, False), "d2_unfused": ((1, 2, 1, 0), 0, False)}


def fit_case(model):
    (p, d, q, I), method, with_init = FIT_MODELS[model]

    def build(engine, dev):
        rows, decoy = _fit_rows(engine)
        N, T = rows.shape
        ui = None
        if with_init:
            ui = _user_init(N, 5)
            ui[70] = [np.nan, np.inf, -np.inf, np.nan, 0.25]
        exp = memo(("fit_exp", model), lambda: oracle_fit(rows, p, d, q, I, method, ui))
        d_rows = In(dev, rows, decoy, ld=T + 3)
        d_ui = In(dev, ui, _user_init(N, 6)) if with_init else None
        outs = fit_outs(dev, N, p + q + I)

        def call(stream):
            engine.fit_batch_device(d_rows.ptr, N, T, d_rows.ld, p, d, q, I, *ptrs(outs),
                                    d_user_init=d_ui.ptr if d_ui else None, method=method, stream=stream,
                                    blocking=False)

        return Scenario([d_rows] + ([d_ui] if d_ui else []), outs, call,
                        lambda got: check_fit(dict(zip(FIT_KEYS, got)), exp, f"fit {model}"))
    return build


def sliced_fit_case(engine, dev):
    p, d, q, I, _ = C1
    N, T = 2049, 48
    d_contig, rows = sampled(engine, N, T, C1, 20261020)
    _, decoy = sampled(engine, N, T, C1, 20261021)
    slices = plan(N, 1024, 0)
    assert slices == [0, 1024, 2048, 2049]                   # fit_slice_bytes 1: 1024-row slices, a tail of one row
    idx = sample_rows(N, [slices])
    exp = memo("sliced_exp", lambda: oracle_fit(rows[idx], p, d, q, I))
    d_rows = In(dev, rows, decoy, ld=T + 3)
    outs = fit_outs(dev, N, 3)
    kept = {}

    def call(stream):
        engine.fit_batch_device(d_rows.ptr, N, T, d_rows.ld, p, d, q, I, *ptrs(outs), stream=stream, blocking=False)

    def check(got):
        kept["res"] = dict(zip(FIT_KEYS, got))
        check_fit(take(kept["res"], idx), exp, "sliced fit vs oracle")
        st = engine.stats()
        assert st["n_series"] == N and st["series_done"] == N, st
        assert st["n_eval"] == int(kept["res"]["n_eval"].sum(dtype=np.int64)), st

    def after():
        assert engine.get_option("fit_slice_bytes") == 0
        whole = device_fit(engine, d_contig, p, d, q, I)     # the unsliced NULL-stream run, every row
        identical(kept["res"], whole, "sliced on a caller stream vs unsliced")

    return Scenario([d_rows], outs, call, check, after)


ORDERS = {"212": (2, 1, 2, 1), "712_runtime": (7, 1, 2, 1)}


def _model_inputs(order):
    p, d, q, I = ORDERS[order]
    k = p + q + I
    return memo(("model_inputs", order), lambda: (
        _walks(300 + p, 65, 97), np.random.default_rng(310 + p).uniform(-0.5, 0.5, (65, k)),
        _walks(320 + p, 65, 97), np.random.default_rng(330 + p).uniform(-0.5, 0.5, (65, k))))


def forecast_case(order):
    p, d, q, I = ORDERS[order]

    def build(engine, dev):
        rows, coef, decoy_rows, decoy_coef = _model_inputs(order)
        N, T, nf = 65, 97, 17
        exp = memo(("forecast_exp", order),
                   lambda: np.stack([O.forecast(rows[i], p, d, q, I, coef[i], nf) for i in range(N)]))
        d_rows, d_coef = In(dev, rows, decoy_rows, ld=T + 3), In(dev, coef, decoy_coef)
        out = Out(dev, N, T + nf, ld=T + nf + 5)

        def call(stream):
            engine.forecast_device(d_rows.ptr, N, T, d_rows.ld, p, d, q, I, d_coef.ptr, nf, out.ptr, out.ld,
                                   stream=stream, blocking=False)

        return Scenario([d_rows, d_coef], [out], call, lambda got: same(got[0], exp, f"forecast {order}"))
    return build


def effects_case(which, order):
    p, d, q, I = ORDERS[order]
    ref = O.remove_time_dependent_effects if which == "remove" else O.add_time_dependent_effects

    def build(engine, dev):
        rows, coef, decoy_rows, decoy_coef = _model_inputs(order)
        N, T = 65, 97
        exp = memo(("effects_exp", which, order),
                   lambda: np.stack([ref(rows[i], p, d, q, I, coef[i]) for i in range(N)]))
        d_rows, d_coef = In(dev, rows, decoy_rows, ld=T + 3), In(dev, coef, decoy_coef)
        out = Out(dev, N, T, ld=T + 5)
        run = engine.remove_effects_device if which == "remove" else engine.add_effects_device

        def call(stream):
            run(d_rows.ptr, N, T, d_rows.ld, p, d, q, I, d_coef.ptr, out.ptr, out.ld, stream=stream, blocking=False)

        return Scenario([d_rows, d_coef], [out], call, lambda got: same(got[0], exp, f"{which} effects {order}"))
    return build


DIAG_N, DIAG_T, DIAG_LAG = 130, 97, 9


def _diag_inputs():
    """Rows, ARIMA(2,1,2)+c coefficients, the restated residuals and the restated diagnostics of rows and residuals."""
    def make():
        rows, coef = _walks(400, DIAG_N, DIAG_T), np.random.default_rng(401).uniform(-0.2, 0.2, (DIAG_N, 5))
        resid = np.stack([O.remove_time_dependent_effects(rows[i], 2, 1, 2, 1, coef[i]) for i in range(DIAG_N)])
        return dict(rows=rows, coef=coef, resid=resid, decoy_rows=_walks(402, DIAG_N, DIAG_T),
                    decoy_coef=np.random.default_rng(403).uniform(-0.2, 0.2, (DIAG_N, 5)),
                    diag_rows=diag_ref(rows, DIAG_LAG), diag_resid=diag_ref(resid, DIAG_LAG))
    return memo("diag_inputs", make)


def diagnostics_case(engine, dev):
    x = _diag_inputs()
    d_rows = In(dev, x["rows"], x["decoy_rows"], ld=DIAG_T + 3)
    outs = diag_outs(dev, DIAG_N, DIAG_LAG)

    def call(stream):
        engine.diagnostics_device(d_rows.ptr, DIAG_N, DIAG_T, d_rows.ld, DIAG_LAG, *ptrs(outs), stream=stream,
                                  blocking=False)

    return Scenario([d_rows], outs, call, lambda got: diag_check(dict(zip(DIAG_KEYS, got)), x["diag_rows"], "diagnostics"))


def residual_diagnostics_case(engine, dev):
    x = _diag_inputs()
    d_rows, d_coef = In(dev, x["rows"], x["decoy_rows"], ld=DIAG_T + 3), In(dev, x["coef"], x["decoy_coef"])
    outs = diag_outs(dev, DIAG_N, DIAG_LAG)

    def call(stream):
        engine.residual_diagnostics_device(d_rows.ptr, DIAG_N, DIAG_T, d_rows.ld, 2, 1, 2, True, d_coef.ptr, DIAG_LAG,
                                           *ptrs(outs), stream=stream, blocking=False)

    return Scenario([d_rows, d_coef], outs, call,
                    lambda got: diag_check(dict(zip(DIAG_KEYS, got)), x["diag_resid"], "residual diagnostics"))


def _search_rows(engine):
    """65 x 64: I(1) rows of the sampler, every third one white noise, so the KPSS choice of d and the grid's pick vary."""
    def make():
        _, rows = sampled(engine, 65, 64, C2, 515)
        rows = rows.copy()
        rows[::3] = np.random.default_rng(516).standard_normal(rows[::3].shape)
        _, decoy = sampled(engine, 65, 64, C2, 517)
        return rows, decoy
    return memo("search_rows", make)


def order_search_case(engine, dev):
    rows, decoy = _search_rows(engine)
    N, T = rows.shape
    exp = memo("search_exp", lambda: O.order_search(rows, 2, 1, 2, 2))
    d_rows = In(dev, rows, decoy, ld=T + 3)
    outs = [Out(dev, N, 4, dtype="int32"), Out(dev, N, 11), Out(dev, N)]

    def call(stream):
        engine.order_search_device(d_rows.ptr, N, T, d_rows.ld, 2, 1, 2, 2, *ptrs(outs), stream=stream, blocking=False)

    def check(got):
        for g, e, name in zip(got, exp, ("order", "coef", "aic")):
            same(g, e, f"order search {name}")

    return Scenario([d_rows], outs, call, check)


AF_KEYS = ("order", "coef", "aic", "status", "n_fits")


def autofit_case(engine, dev):
    rows, decoy = _search_rows(engine)
    N, T = rows.shape

    def make():
        fits = [O.autofit(r, 2, 1, 2) for r in rows]
        return {k: np.array([f[k] for f in fits]) for k in AF_KEYS}
    exp = memo("autofit_exp", make)
    d_rows = In(dev, rows, decoy, ld=T + 3)
    outs = [Out(dev, N, 4, dtype="int32"), Out(dev, N, 11), Out(dev, N), Out(dev, N, dtype="int32"),
            Out(dev, N, dtype="int32")]

    def call(stream):
        engine.autofit_device(d_rows.ptr, N, T, d_rows.ld, 2, 1, 2, *ptrs(outs), stream=stream, blocking=False)

    return Scenario([d_rows], outs, call, lambda got: check_autofit(dict(zip(AF_KEYS, got)), exp, "autofit"))


def sample_case(engine, dev):
    # the one entry point with no CPU restatement of its noise: against its own blocking NULL-stream output
    p, d, q, I, base = C2
    N, T, seed, first = 130, 97, 20261020, 1000
    exp = memo("sample_exp", lambda: _device_sample(engine, N, T, p, d, q, I, base, 0.05, seed, first).cpu().numpy())
    out = Out(dev, N, T, ld=T + 3)

    def call(stream):
        engine.sample_device(out.ptr, N, T, out.ld, p, d, q, I, base, 0.05, seed, first, stream=stream, blocking=False)

    return Scenario([], [out], call, lambda got: same(got[0], exp, "sample"))


def model_fit_case(name):
    def build(engine, dev):
        meta, arr = load_case(name)
        model = meta.get("model", "argarch")
        rows = arr["series"]
        N, T = rows.shape
        decoy = np.random.default_rng(len(name)).standard_normal((N, T)) * 0.5
        d_rows = In(dev, rows, decoy, ld=T + 3)
        outs = model_outs(dev, N, L.MODEL_PARAMS[model])
        fit = getattr(engine, f"{model}_fit_batch_device")

        def call(stream):
            fit(d_rows.ptr, N, T, d_rows.ld, *ptrs(outs), stream=stream, blocking=False)

        def check(got):
            for g, key in zip(got, MODEL_KEYS):
                same(g, arr[key], f"{name} {key}")

        return Scenario([d_rows], outs, call, check)
    return build


def _pairs():
    """argarch_ref.pair_reference(97) (rows, ARGARCH and AR parameters, their expected outputs) plus smallfit_ref's EWMA
    and GARCH pairs over the same rows, and decoys for rows and parameters."""
    def make():
        ref = dict(AR.pair_reference(97))
        N = ref["rows"].shape[0]
        rng = np.random.default_rng(99)
        sm = rng.uniform(0.05, 1.5, N)
        sm[:4] = (-0.3, 1.7, np.nan, 0.0)                    # outside (0, 1), a NaN, and remove's division by zero
        ref["sm"] = sm
        rl, gl, sl = ref["rows"].tolist(), ref["g"][:, 2:].tolist(), sm.tolist()
        ref["ewma_remove"] = np.array([SR.ewma_remove(r, a) for r, a in zip(rl, sl)])
        ref["ewma_add"] = np.array([SR.ewma_add(r, a) for r, a in zip(rl, sl)])
        ref["garch_remove"] = np.array([SR.garch_remove(r, *c) for r, c in zip(rl, gl)])
        ref["garch_add"] = np.array([SR.garch_add(r, *c) for r, c in zip(rl, gl)])
        ref["decoy_rows"] = np.random.default_rng(98).standard_normal(ref["rows"].shape)
        return ref
    return memo("pairs", make)


def pair_case(kind, arg, direction=None):
    """kind "model" (arg ewma / garch / argarch), "ar" (arg p) or "sample" (arg garch / argarch)."""
    def build(engine, dev):
        ref = _pairs()
        N, T = ref["rows"].shape
        if kind == "ar":
            params, want = ref["ar"][arg], ref[f"ar_{direction}_{arg}"]
        elif kind == "sample":
            params, want = (ref["g"][:, 2:] if arg == "garch" else ref["g"]), ref[f"{arg}_sample"]
        else:
            params = {"ewma": ref["sm"], "garch": ref["g"][:, 2:], "argarch": ref["g"]}[arg]
            want = ref[f"{arg}_{direction}"]
        decoy = np.random.default_rng(97).uniform(0.05, 0.4, params.shape)
        d_rows, d_par = In(dev, ref["rows"], ref["decoy_rows"], ld=T + 3), In(dev, params, decoy)
        out = Out(dev, N, T, ld=T + 5)

        def call(stream):
            tail = dict(stream=stream, blocking=False)
            if kind == "ar":
                engine.ar_effects_device(direction, d_rows.ptr, N, T, d_rows.ld, arg, d_par.ptr, out.ptr, out.ld, **tail)
            elif kind == "sample":
                engine.model_sample_device(arg, d_rows.ptr, N, T, d_rows.ld, d_par.ptr, out.ptr, out.ld, **tail)
            else:
                engine.model_effects_device(arg, direction, d_rows.ptr, N, T, d_rows.ld, d_par.ptr, out.ptr, out.ld,
                                            **tail)

        return Scenario([d_rows, d_par], [out], call, lambda got: same(got[0], want, f"{kind} {arg} {direction}"))
    return build


RG_N, RG_T, RG_LAG = 70, 40, 2
RG_CFG = (3, 2, 3, True, False)         # yMaxLag, xMaxLag, k, includeOriginalX, noIntercept: K = 12, R = 37


def _regress_inputs():
    """70 rows of tests/test_gpu_regress.py's batch of RG_CFG with its restated fits and predictions, the restated
    bgtest and bptest of the same rows, and decoys. x: per series k rows of T values."""
    def make():
        k = RG_CFG[2]
        y, x, coef, status, pred = (a[:RG_N] for a in _arx_case(RG_CFG))
        rng = np.random.default_rng(440)
        return dict(y=y, x=np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(RG_N, k * RG_T), coef=coef, status=status,
                    pred=pred, bg=[RR.bgtest(y[i], x[i].T, RG_LAG) for i in range(RG_N)],
                    bp=[RR.bptest(y[i], x[i].T) for i in range(RG_N)], decoy_y=_walks(441, RG_N, RG_T),
                    decoy_x=rng.standard_normal((RG_N, k * RG_T)), decoy_coef=rng.uniform(-0.5, 0.5, coef.shape))
    return memo("regress_inputs", make)


def _regress_sources(dev, r):
    """The rows (ld = T + 3) and the regressors (a series stride of k T + 5) and the arguments that name them."""
    k = RG_CFG[2]
    d_y, d_x = In(dev, r["y"], r["decoy_y"], ld=RG_T + 3), In(dev, r["x"], r["decoy_x"], ld=k * RG_T + 5)
    return d_y, d_x, (d_y.ptr, RG_N, RG_T, d_y.ld, d_x.ptr, d_x.ld, k)


def regress_case(which):
    """which: arx_fit, arx_predict, bgtest or bptest."""
    def build(engine, dev):
        r = _regress_inputs()
        yl, xl, k, orig, noint = RG_CFG
        d_y, d_x, head = _regress_sources(dev, r)
        if which == "arx_fit":
            outs = [Out(dev, RG_N, 1 + yl + k * xl + k), Out(dev, RG_N, dtype="int32")]

            def call(stream):
                engine.arx_fit_device(*head, yl, xl, orig, noint, *ptrs(outs), stream=stream, blocking=False)

            def check(got):
                same(got[0], r["coef"], "arx fit coef")
                same(got[1], r["status"], "arx fit status")

            return Scenario([d_y, d_x], outs, call, check)
        if which == "arx_predict":
            d_coef = In(dev, r["coef"], r["decoy_coef"])
            rows = RG_T - max(yl, xl)
            out = Out(dev, RG_N, rows, ld=rows + 5)

            def call(stream):
                engine.arx_predict_device(*head, yl, xl, orig, d_coef.ptr, out.ptr, out.ld, stream=stream, blocking=False)

            return Scenario([d_y, d_x, d_coef], [out], call, lambda got: same(got[0], r["pred"], "arx predict"))
        outs = [Out(dev, RG_N), Out(dev, RG_N), Out(dev, RG_N, dtype="int32")]
        ref = r["bg" if which == "bgtest" else "bp"]

        def call(stream):
            if which == "bgtest":
                engine.bgtest_device(*head, RG_LAG, *ptrs(outs), stream=stream, blocking=False)
            else:
                engine.bptest_device(*head, *ptrs(outs), stream=stream, blocking=False)

        def check(got):
            same(got[0], np.array([x[1] for x in ref]), f"{which} statistic")
            assert _p_close(got[1], [x[2] for x in ref]), f"{which} p-value"
            same(got[2], np.array([x[0] for x in ref], dtype=np.int32), f"{which} status")

        return Scenario([d_y, d_x], outs, call, check)
    return build


def _cases():
    c = []
    for model in FIT_MODELS:
        for P in (1, 3):
            c.append(pytest.param(fit_case(model), dict(fit_pipeline=P), id=f"fit-{model}-pipeline{P}"))
    c.append(pytest.param(sliced_fit_case, dict(fit_slice_bytes=1), id="fit-sliced-3-slices"))
    for order in ORDERS:
        c.append(pytest.param(forecast_case(order), {}, id=f"forecast-{order}"))
        for which in ("remove", "add"):
            c.append(pytest.param(effects_case(which, order), {}, id=f"{which}_effects-{order}"))
    c.append(pytest.param(diagnostics_case, {}, id="diagnostics"))
    c.append(pytest.param(residual_diagnostics_case, dict(diag_slice_bytes=1), id="residual_diagnostics-3-slices"))
    for lanes in (1, 4):
        c.append(pytest.param(order_search_case, dict(search_lanes=lanes), id=f"order_search-lanes{lanes}"))
    for sl in (0, 32):
        c.append(pytest.param(autofit_case, dict(autofit_slice=sl), id=f"autofit-slice{sl}"))
    c.append(pytest.param(sample_case, {}, id="sample"))
    for name in SR.FIXTURES + ("argarch/argarch_T97",):
        c.append(pytest.param(model_fit_case(name), {}, id="model_fit-" + name.split("/")[1]))
    for model in ("ewma", "garch", "argarch"):
        for direction in ("remove", "add"):
            c.append(pytest.param(pair_case("model", model, direction), {}, id=f"{model}_{direction}_effects"))
    for p in (1, 20):
        for direction in ("remove", "add"):
            c.append(pytest.param(pair_case("ar", p, direction), {}, id=f"ar_{direction}_effects-p{p}"))
    for model in ("garch", "argarch"):
        c.append(pytest.param(pair_case("sample", model), {}, id=f"{model}_sample"))
    for which in ("arx_fit", "arx_predict"):
        c.append(pytest.param(regress_case(which), {}, id=which))
    for which in ("bgtest", "bptest"):                         # 70 series in slices of 64: the slice loop on the caller's stream
        c.append(pytest.param(regress_case(which), dict(regress_slice_bytes=1), id=f"{which}-2-slices"))
    return c


_rotation = [0]


@pytest.mark.parametrize("build,opts", _cases())
def test_entry_point_on_caller_stream(engine, rig, build, opts, request):
    sc = build(engine, rig.dev)
    s = rig.streams[_rotation[0] % 3]
    _rotation[0] += 1
    with options(engine, **opts):
        got = run_scenario(rig, s, sc, request.node.callspec.id)
        sc.check(got)
    if sc.after:
        sc.after()


# ---- 2. ordering across streams on one handle ---------------------------------------------------------------------------
def test_sample_then_fit_across_streams(engine, rig):
    # non-fit -> fit: the sampler writes the rows on one stream, the fit reads them on another
    torch = rig.torch
    p, d, q, I, base = C2
    N, T, seed = 130, 100, 4711
    d_contig, rows = sampled(engine, N, T, C2, seed)          # the serial chain's first link (no CPU restatement)
    serial = device_fit(engine, d_contig, p, d, q, I)        # its second link, held to the oracle
    check_fit(serial, memo("chain_fit_exp", lambda: oracle_fit(rows, p, d, q, I)), "serial sample -> fit")
    _, decoy = _fit_rows(engine)
    buf = In(rig.dev, rows, decoy, ld=T + 3)                 # holds the decoys; the sampler overwrites them
    outs = fit_outs(rig.dev, N, 5)
    s1, s2 = rig.chain(0, 1)
    torch.cuda.synchronize(rig.dev)
    with torch.cuda.stream(s1):
        rig.delay()
        engine.sample_device(buf.ptr, N, T, buf.ld, p, d, q, I, base, 0.05, seed, 0, stream=s1.cuda_stream,
                             blocking=False)
    with torch.cuda.stream(s2):
        engine.fit_batch_device(buf.ptr, N, T, buf.ld, p, d, q, I, *ptrs(outs), stream=s2.cuda_stream, blocking=False)
        snaps, in_snap = snapshots(outs), buf.full.clone()
    s2.synchronize()
    got = dict(zip(FIT_KEYS, bodies(rig, s2, outs, snaps, "sample -> fit")))
    identical(got, serial, "sample on one stream, fit on another")
    buf.untouched(rig.host(in_snap, s2), "sampled rows")
    s1.synchronize()


def test_fit_then_consumers_across_streams(engine, rig):
    # fit -> non-fit: the fit's coefficients feed forecast, remove_effects and residual_diagnostics on another stream
    torch = rig.torch
    p, d, q, I, _ = C2
    N, T, nf, lag = 130, 100, 17, DIAG_LAG
    rows, decoy = _fit_rows(engine)
    d_contig, _ = sampled(engine, N, T, C2, 4711)

    def serial_chain():
        fit = device_fit(engine, d_contig, p, d, q, I)
        check_fit(fit, memo("chain_fit_exp", lambda: oracle_fit(rows, p, d, q, I)), "serial fit")
        coef = torch.from_numpy(np.ascontiguousarray(fit["coef"])).to(rig.dev)
        fc = torch.empty((N, T + nf), dtype=torch.float64, device=rig.dev)
        res = torch.empty((N, T), dtype=torch.float64, device=rig.dev)
        dg = [torch.empty((N, lag), dtype=torch.float64, device=rig.dev)] + \
            [torch.empty(N, dtype=torch.float64, device=rig.dev) for _ in range(3)]
        engine.forecast_device(d_contig.data_ptr(), N, T, T, p, d, q, I, coef.data_ptr(), nf, fc.data_ptr(), T + nf)
        engine.remove_effects_device(d_contig.data_ptr(), N, T, T, p, d, q, I, coef.data_ptr(), res.data_ptr(), T)
        engine.residual_diagnostics_device(d_contig.data_ptr(), N, T, T, p, d, q, I, coef.data_ptr(), lag,
                                           *[t.data_ptr() for t in dg])
        out = dict(fit=fit, fc=fc.cpu().numpy(), res=res.cpu().numpy(), dg=[t.cpu().numpy() for t in dg])
        ok = np.nonzero(fit["status"] == 0)[0]               # a failed fit has no model to restate
        assert ok.size > N // 2
        c = fit["coef"]
        same(out["fc"][ok], np.stack([O.forecast(rows[i], p, d, q, I, c[i], nf) for i in ok]), "serial forecast")
        resid = np.stack([O.remove_time_dependent_effects(rows[i], p, d, q, I, c[i]) for i in ok])
        same(out["res"][ok], resid, "serial residuals")
        diag_check({k: v[ok] for k, v in zip(DIAG_KEYS, out["dg"])}, diag_ref(resid, lag), "serial residual diagnostics")
        return out
    serial = memo("fit_consumers_serial", serial_chain)

    d_rows = In(rig.dev, rows, decoy, ld=T + 3)
    f_outs = fit_outs(rig.dev, N, 5)
    fc, res, dg = Out(rig.dev, N, T + nf, ld=T + nf + 5), Out(rig.dev, N, T, ld=T + 5), diag_outs(rig.dev, N, lag)
    coef = f_outs[0].ptr
    s1, s2 = rig.chain(0, 1)
    torch.cuda.synchronize(rig.dev)
    with torch.cuda.stream(s1):
        rig.delay()
        d_rows.load()
        engine.fit_batch_device(d_rows.ptr, N, T, d_rows.ld, p, d, q, I, *ptrs(f_outs), stream=s1.cuda_stream,
                                blocking=False)
    with torch.cuda.stream(s2):
        tail = dict(stream=s2.cuda_stream, blocking=False)
        engine.forecast_device(d_rows.ptr, N, T, d_rows.ld, p, d, q, I, coef, nf, fc.ptr, fc.ld, **tail)
        engine.remove_effects_device(d_rows.ptr, N, T, d_rows.ld, p, d, q, I, coef, res.ptr, res.ld, **tail)
        engine.residual_diagnostics_device(d_rows.ptr, N, T, d_rows.ld, p, d, q, I, coef, lag, *ptrs(dg), **tail)
        outs = f_outs + [fc, res] + dg
        snaps = snapshots(outs)
    s2.synchronize()
    got = bodies(rig, s2, outs, snaps, "fit -> consumers")
    identical(dict(zip(FIT_KEYS, got[:6])), serial["fit"], "the fit")
    same(got[6], serial["fc"], "forecast of the fit's coefficients")
    same(got[7], serial["res"], "residuals under the fit's coefficients")
    for g, e, k in zip(got[8:], serial["dg"], DIAG_KEYS):
        same(g, e, f"residual diagnostics {k}")
    s1.synchronize()


def test_remove_effects_then_diagnostics_across_streams(engine, rig):
    # non-fit -> non-fit: the residuals written on one stream are the rows of the diagnostics on another
    torch = rig.torch
    x = _diag_inputs()
    N, T, lag = DIAG_N, DIAG_T, DIAG_LAG

    def serial_chain():
        rows, coef = torch.from_numpy(x["rows"]).to(rig.dev), torch.from_numpy(x["coef"]).to(rig.dev)
        res = torch.empty((N, T), dtype=torch.float64, device=rig.dev)
        dg = [torch.empty((N, lag), dtype=torch.float64, device=rig.dev)] + \
            [torch.empty(N, dtype=torch.float64, device=rig.dev) for _ in range(3)]
        engine.remove_effects_device(rows.data_ptr(), N, T, T, 2, 1, 2, 1, coef.data_ptr(), res.data_ptr(), T)
        engine.diagnostics_device(res.data_ptr(), N, T, T, lag, *[t.data_ptr() for t in dg])
        out = dict(res=res.cpu().numpy(), dg=[t.cpu().numpy() for t in dg])
        same(out["res"], x["resid"], "serial residuals")
        diag_check(dict(zip(DIAG_KEYS, out["dg"])), x["diag_resid"], "serial diagnostics")
        return out
    serial = memo("remove_diag_serial", serial_chain)

    d_rows, d_coef = In(rig.dev, x["rows"], x["decoy_rows"], ld=T + 3), In(rig.dev, x["coef"], x["decoy_coef"])
    mid, dg = Out(rig.dev, N, T, ld=T + 5), diag_outs(rig.dev, N, lag)
    s1, s2 = rig.chain(1, 2)
    torch.cuda.synchronize(rig.dev)
    with torch.cuda.stream(s1):
        rig.delay()
        d_rows.load()
        d_coef.load()
        engine.remove_effects_device(d_rows.ptr, N, T, d_rows.ld, 2, 1, 2, 1, d_coef.ptr, mid.ptr, mid.ld,
                                     stream=s1.cuda_stream, blocking=False)
    with torch.cuda.stream(s2):
        engine.diagnostics_device(mid.ptr, N, T, mid.ld, lag, *ptrs(dg), stream=s2.cuda_stream, blocking=False)
        outs = [mid] + dg
        snaps = snapshots(outs)
    s2.synchronize()
    got = bodies(rig, s2, outs, snaps, "remove -> diagnostics")
    same(got[0], serial["res"], "residuals")
    for g, e, k in zip(got[1:], serial["dg"], DIAG_KEYS):
        same(g, e, f"diagnostics {k}")
    s1.synchronize()


def test_ar_residuals_then_garch_fit_across_streams(engine, rig):
    # non-fit -> non-fit: ARModel's residuals on one stream, their GARCH fit on another; the result is the GARCH part of
    # the fused ARGARCH fit (tests/test_gpu_argarch.py test_fused_equals_unfused_chain), here from the committed golden
    torch = rig.torch
    meta, arr = load_case("argarch/argarch_T97")
    ok = arr["ar_status"] == 0                               # a row whose AR stage failed has no residuals
    rows = np.ascontiguousarray(arr["series"][ok])
    N, T = rows.shape
    assert meta["N"] == 130 and 65 < N < 130

    def restated():
        ar = np.empty((N, 2))
        for i, r in enumerate(rows.tolist()):
            st, c, phi = O.ar_fit(r, 1)
            assert st == 0
            ar[i] = (c, float(phi[0]))
        return ar, np.array([AR.ar_remove(r, a[0], [a[1]]) for r, a in zip(rows.tolist(), ar.tolist())])
    ar, resid = memo("ar_garch_restated", restated)
    want = dict(coef=arr["coef"][ok][:, 2:], obj=arr["obj"][ok], status=arr["status"][ok], n_eval=arr["n_eval"][ok],
                n_grad=arr["n_grad"][ok])

    def serial_chain():
        d_rows, d_ar = torch.from_numpy(rows).to(rig.dev), torch.from_numpy(ar).to(rig.dev)
        res = torch.empty((N, T), dtype=torch.float64, device=rig.dev)
        r = [torch.empty((N, 3), dtype=torch.float64, device=rig.dev), torch.empty(N, dtype=torch.float64, device=rig.dev)] + \
            [torch.empty(N, dtype=torch.int32, device=rig.dev) for _ in range(3)]
        engine.ar_effects_device("remove", d_rows.data_ptr(), N, T, T, 1, d_ar.data_ptr(), res.data_ptr(), T)
        engine.garch_fit_batch_device(res.data_ptr(), N, T, T, *[t.data_ptr() for t in r])
        out = dict(res=res.cpu().numpy(), fit=dict(zip(MODEL_KEYS, [t.cpu().numpy() for t in r])))
        same(out["res"], resid, "serial AR residuals")
        for k in MODEL_KEYS:
            same(out["fit"][k], want[k], f"serial GARCH fit {k}")
        return out
    serial = memo("ar_garch_serial", serial_chain)

    rng = np.random.default_rng(7)
    d_rows = In(rig.dev, rows, rng.standard_normal((N, T)), ld=T + 3)
    d_ar = In(rig.dev, ar, rng.uniform(-0.5, 0.5, (N, 2)))
    mid, outs = Out(rig.dev, N, T, ld=T + 5), model_outs(rig.dev, N, 3)
    s1, s2 = rig.chain(2, 0)
    torch.cuda.synchronize(rig.dev)
    with torch.cuda.stream(s1):
        rig.delay()
        d_rows.load()
        d_ar.load()
        engine.ar_effects_device("remove", d_rows.ptr, N, T, d_rows.ld, 1, d_ar.ptr, mid.ptr, mid.ld,
                                 stream=s1.cuda_stream, blocking=False)
    with torch.cuda.stream(s2):
        engine.garch_fit_batch_device(mid.ptr, N, T, mid.ld, *ptrs(outs), stream=s2.cuda_stream, blocking=False)
        snaps = snapshots([mid] + outs)
    s2.synchronize()
    got = bodies(rig, s2, [mid] + outs, snaps, "AR residuals -> GARCH fit")
    same(got[0], serial["res"], "AR residuals")
    for g, k in zip(got[1:], MODEL_KEYS):
        same(g, serial["fit"][k], f"GARCH fit {k}")
        same(g, want[k], f"GARCH part of the fused fit {k}")
    s1.synchronize()


def test_arx_fit_then_predict_across_streams(engine, rig):
    # non-fit -> non-fit: the regression writes its coefficients on one stream, ARXModel.predict reads them on another
    torch = rig.torch
    r = _regress_inputs()
    yl, xl, k, orig, noint = RG_CFG
    d_y, d_x, head = _regress_sources(rig.dev, r)
    rows = RG_T - max(yl, xl)
    f_outs = [Out(rig.dev, RG_N, 1 + yl + k * xl + k), Out(rig.dev, RG_N, dtype="int32")]
    pred = Out(rig.dev, RG_N, rows, ld=rows + 5)
    s1, s2 = rig.chain(1, 2)
    torch.cuda.synchronize(rig.dev)
    with torch.cuda.stream(s1):
        rig.delay()
        d_y.load()
        d_x.load()
        engine.arx_fit_device(*head, yl, xl, orig, noint, *ptrs(f_outs), stream=s1.cuda_stream, blocking=False)
    with torch.cuda.stream(s2):
        engine.arx_predict_device(*head, yl, xl, orig, f_outs[0].ptr, pred.ptr, pred.ld, stream=s2.cuda_stream,
                                  blocking=False)
        outs = f_outs + [pred]
        snaps, in_snaps = snapshots(outs), snapshots([d_y, d_x])
    s2.synchronize()
    got = bodies(rig, s2, outs, snaps, "arx fit -> predict")
    same(got[0], r["coef"], "the fit's coefficients")
    same(got[1], r["status"], "the fit's status")
    assert np.all(r["status"] == RR.ST_OK)
    same(got[2], r["pred"], "the prediction at the fit's coefficients")        # regress_ref's, at the real coefficients
    for i, x in zip((d_y, d_x), in_snaps):
        i.untouched(rig.host(x, s2), "arx fit -> predict")
    s1.synchronize()


PIPE_N, PIPE_T = 2048, 128


def _pipe_rows(engine, seed):
    return sampled(engine, PIPE_N, PIPE_T, C2, seed)


def _plain_outs(torch, dev, N, k):
    return [torch.empty((N, k), dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.float64, device=dev)] + \
        [torch.empty(N, dtype=torch.int32, device=dev) for _ in range(3)] + [torch.empty(N, dtype=torch.uint8, device=dev)]


def test_pipelined_fits_that_share_buffers_stay_ordered_across_streams(engine, rig):
    # fit -> fit under fit_pipeline 3: the read-after-write / write-after-read / write-after-write scenario of
    # tests/test_gpu_parity.py test_pipelined_fits_that_share_buffers_stay_ordered with consecutive calls on s1, s2, s3,
    # s1, s2, against the same scenario under fit_pipeline 1 on the NULL stream
    torch = rig.torch
    N, T = PIPE_N, PIPE_T
    (d1, h1), (d2, h2) = _pipe_rows(engine, 71), _pipe_rows(engine, 72)

    def scenario(streams):
        """streams None: every call on the NULL stream and the handle synchronised at the end (the serial reference)."""
        a, b, c, zl = (_plain_outs(torch, rig.dev, N, 5) for _ in range(4))
        z = d2.clone()
        zl[1] = z[:, 0]                    # the fourth call writes its ll over z's first N doubles
        torch.cuda.synchronize(rig.dev)
        calls = [(d1, a, None), (d2, b, a[0]),     # RAW: b starts from a's coefficients
                 (z, c, None), (d1, zl, None),     # WAR: c reads z while the next call writes into it
                 (d1, b, None)]                    # WAW: b's buffers rewritten by a fit of d1
        for i, (series, o, init) in enumerate(calls):
            s = None if streams is None else streams[i % 3]
            with contextlib.nullcontext() if s is None else torch.cuda.stream(s):
                if i == 0 and s is not None:
                    rig.delay()
                engine.fit_batch_device(series.data_ptr(), N, T, T, 2, 1, 2, 1, *[t.data_ptr() for t in o],
                                        d_user_init=None if init is None else init.data_ptr(),
                                        stream=None if s is None else s.cuda_stream, blocking=False)
        if streams is None:
            engine.synchronize()
            return [[t.cpu().numpy() for t in r] for r in (a, b, c)]
        # a's last writer ran on s1, b's on s2, c's on s3: each is snapshot and read through that stream alone
        snaps = []
        for s, r in zip(streams, (a, b, c)):
            with torch.cuda.stream(s):
                snaps.append([t.clone() for t in r])
        out = []
        for s, r in zip(streams, snaps):
            s.synchronize()
            out.append([rig.host(t, s) for t in r])
        return out

    with options(engine, fit_pipeline=1):
        serial = memo("pipe_serial", lambda: scenario(None))
    idx = sample_rows(N, [[0, N]])
    for res, host, what in ((serial[0], h1, "a"), (serial[2], h2, "c")):       # the links, held to the oracle
        exp = memo(("pipe_exp", what), lambda: oracle_fit(host[idx], 2, 1, 2, 1))
        check_fit(take(dict(zip(FIT_KEYS, res)), idx), exp, f"serial {what}")
    with options(engine, fit_pipeline=3):
        piped = scenario(rig.chain(0, 1, 2, 0, 1)[:3])
    for ra, rb, what in zip(serial, piped, "abc"):
        for x, y, k in zip(ra, rb, FIT_KEYS):
            same(y, x, f"{what} {k}")
    for x, y, k in zip(piped[0], piped[1], FIT_KEYS):
        same(y, x, f"the WAW's final contents {k}")                             # d1's fit, as the first call's


def test_independent_pipelined_fits_across_streams(engine, rig):
    # fit_pipeline 3: five independent fits of different orders, one per stream in rotation, each equal to its serial
    # (fit_pipeline 1, NULL stream, blocking) result
    torch = rig.torch
    N, T = PIPE_N, PIPE_T
    d1, h1 = _pipe_rows(engine, 71)
    orders = [(2, 1, 2, 1), (1, 1, 1, 1), (2, 1, 2, 1), (3, 1, 2, 0), (2, 1, 2, 1)]
    idx = sample_rows(N, [[0, N]])

    def serial_fits():
        out = {}
        for o in sorted(set(orders)):
            out[o] = device_fit(engine, d1, *o)
            check_fit(take(out[o], idx), oracle_fit(h1[idx], *o), f"serial {o}")
        return out
    with options(engine, fit_pipeline=1):
        serial = memo("independent_serial", serial_fits)
    streams = rig.chain(0, 1, 2)
    outs = [_plain_outs(torch, rig.dev, N, p + q + I) for p, d, q, I in orders]
    torch.cuda.synchronize(rig.dev)
    snaps = []
    with options(engine, fit_pipeline=3):
        for i, ((p, d, q, I), o) in enumerate(zip(orders, outs)):
            s = streams[i % 3]
            with torch.cuda.stream(s):
                if i == 0:
                    rig.delay()
                engine.fit_batch_device(d1.data_ptr(), N, T, T, p, d, q, I, *[t.data_ptr() for t in o],
                                        stream=s.cuda_stream, blocking=False)
                snaps.append([t.clone() for t in o])
    for s in streams:
        s.synchronize()
    for i, (o, r) in enumerate(zip(orders, snaps)):
        got = dict(zip(FIT_KEYS, [rig.host(t, streams[i % 3]) for t in r]))
        identical(got, serial[o], f"fit {i} {o}")


def test_synchronize_makes_results_visible_to_the_host(engine, rig):
    # the host's view: after a non-blocking fit behind the delay, arima_synchronize alone (the stream is not
    # synchronised) makes the results readable through torch's default stream
    torch = rig.torch
    p, d, q, I, _ = C2
    rows, decoy = _fit_rows(engine)
    N, T = rows.shape
    exp = memo("chain_fit_exp", lambda: oracle_fit(rows, p, d, q, I))
    d_rows, outs = In(rig.dev, rows, decoy, ld=T + 3), fit_outs(rig.dev, N, 5)
    s1, = rig.chain(0)
    torch.cuda.synchronize(rig.dev)
    with torch.cuda.stream(s1):
        rig.delay()
        d_rows.load()
        engine.fit_batch_device(d_rows.ptr, N, T, d_rows.ld, p, d, q, I, *ptrs(outs), stream=s1.cuda_stream,
                                blocking=False)
    engine.synchronize()
    got = [o.body(o.full.cpu().numpy(), "after synchronize") for o in outs]
    check_fit(dict(zip(FIT_KEYS, got)), exp, "fit read after arima_synchronize")
    s1.synchronize()


def test_stats_wait_for_the_last_call(engine, rig):
    # arima_get_last_stats / arima_get_last_model_fit_stats straight after a non-blocking fit behind the delay return
    # that call's counters
    torch = rig.torch
    p, d, q, I, _ = C2
    rows, decoy = _fit_rows(engine)
    N, T = rows.shape
    d_rows, outs = In(rig.dev, rows, decoy, ld=T + 3), fit_outs(rig.dev, N, 5)
    meta, arr = load_case("smallfit/garch_T97")
    gN, gT = arr["series"].shape
    g_rows = In(rig.dev, arr["series"], np.random.default_rng(3).standard_normal((gN, gT)) * 0.5, ld=gT + 3)
    g_outs = model_outs(rig.dev, gN, 3)
    s1, = rig.chain(0)
    torch.cuda.synchronize(rig.dev)
    with torch.cuda.stream(s1):
        rig.delay()
        d_rows.load()
        engine.fit_batch_device(d_rows.ptr, N, T, d_rows.ld, p, d, q, I, *ptrs(outs), stream=s1.cuda_stream,
                                blocking=False)
        st = engine.stats()
        snaps = snapshots(outs)
        rig.delay()
        g_rows.load()
        engine.garch_fit_batch_device(g_rows.ptr, gN, gT, g_rows.ld, *ptrs(g_outs), stream=s1.cuda_stream,
                                      blocking=False)
        mst = engine.model_fit_stats()
        g_snaps = snapshots(g_outs)
    s1.synchronize()
    got = dict(zip(FIT_KEYS, bodies(rig, s1, outs, snaps, "fit")))
    check_fit(got, memo("chain_fit_exp", lambda: oracle_fit(rows, p, d, q, I)), "fit before stats")
    assert st["n_series"] == N and st["series_done"] == N, st
    assert st["n_eval"] == int(got["n_eval"].sum(dtype=np.int64)), (st["n_eval"], int(got["n_eval"].sum()))
    assert st["n_grad"] == int(got["n_grad"].sum(dtype=np.int64)), st
    g = dict(zip(MODEL_KEYS, bodies(rig, s1, g_outs, g_snaps, "garch fit")))
    for k in MODEL_KEYS:
        same(g[k], arr[k], f"garch fit before model_fit_stats: {k}")
    # the model counters keep no evaluation count: lane_passes is the kernel's own sum of passes, one per posted point
    # (tests/test_gpu_smallfit.py test_fit_parity_host states the relation to the n_eval output)
    good = g["status"] == 0
    n_ok, n_bad = int(g["n_eval"][good].sum()), int(g["n_eval"][~good].sum())
    assert mst["n_series"] == gN, mst
    assert n_ok <= mst["lane_passes"] - n_bad <= n_ok + 4, (mst, n_ok, n_bad)
    assert mst["max_wave_passes"] <= mst["wave_passes"] <= mst["lane_passes"] <= 64 * mst["wave_passes"], mst


# ---- 3. one handle from several host threads ----------------------------------------------------------------------------
@pytest.fixture
def handles(engine):
    """Fresh handles on the engine's device (made on demand), destroyed at the end."""
    made = []

    def make():
        made.append(L.Engine(engine.device))
        return made[-1]
    yield make
    for e in made:
        assert e.L.arima_destroy(e.h) == 0


def run_threads(jobs):
    """Every job on a daemon thread of its own, started together; a deadlock fails the test, an exception is re-raised."""
    barrier = threading.Barrier(len(jobs))
    results, errors = [None] * len(jobs), [None] * len(jobs)

    def body(i):
        try:
            barrier.wait(JOIN_S)
            results[i] = jobs[i]()
        except BaseException as e:       # noqa: BLE001 -- handed to the test
            errors[i] = e

    threads = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_S)
    assert not any(t.is_alive() for t in threads), "a thread is still inside the library after 120 s: deadlock"
    for e in errors:
        if e is not None:
            raise e
    return results


TH_N, TH_T, TH_LAG = 65, 97, 3
TH_OFFSETS = (0, 21, 42, 65)             # each thread's 65-row window of the 130-row references


class Worker:
    """One thread's inputs (its own seed), buffers and stream, allocated before any thread runs. run(engine) issues the
    fixed sequence of host-buffer and device calls and returns every result; expect() is the restatement of each."""

    def __init__(self, engine, rig, i):
        torch = rig.torch
        self.rig, self.i, self.dev = rig, i, rig.dev
        self.stream = torch.cuda.Stream(rig.dev)
        p, d, q, I, base = C1
        N, T = TH_N, TH_T
        self.rows = sampled(engine, N, T, C1, 9000 + i)[1]
        self.coef = np.asarray(base)[None, :] + np.random.default_rng(9100 + i).uniform(-0.1, 0.1, (N, 3))
        off = TH_OFFSETS[i]
        self.garch = load_case("smallfit/garch_T97")[1]
        self.grows = np.ascontiguousarray(self.garch["series"][off:off + N])
        self.pairs = AR.pair_reference(97)
        self.prow = np.ascontiguousarray(self.pairs["rows"][off:off + N])
        self.pg = np.ascontiguousarray(self.pairs["g"][off:off + N])
        self.off = off
        self.seed = 9200 + i

    def buffers(self):
        """Fresh device buffers for one run of the sequence (made on the main thread)."""
        N, T = TH_N, TH_T
        rng = np.random.default_rng(9300 + self.i)
        b = dict(rows=In(self.dev, self.rows, rng.standard_normal((N, T)).cumsum(axis=1), ld=T + 3),
                 coef=In(self.dev, self.coef, rng.uniform(-0.3, 0.3, (N, 3))),
                 grows=In(self.dev, self.grows, rng.standard_normal((N, T)) * 0.5, ld=T + 3),
                 fit=fit_outs(self.dev, N, 3), fc=Out(self.dev, N, T + 5, ld=T + 10), res=Out(self.dev, N, T, ld=T + 5),
                 dg=diag_outs(self.dev, N, TH_LAG), gfit=model_outs(self.dev, N, 3), smp=Out(self.dev, N, T, ld=T + 3))
        return b

    def run(self, engine, b):
        torch = self.rig.torch
        p, d, q, I, base = C1
        N, T, s = TH_N, TH_T, self.stream
        tail = dict(stream=s.cuda_stream, blocking=False)
        r, snaps = {}, {}
        with torch.cuda.stream(s):
            for x in ("rows", "coef", "grows"):
                b[x].load()
            r["host_fit"] = engine.fit_batch(self.rows, p, d, q, True)
            engine.fit_batch_device(b["rows"].ptr, N, T, b["rows"].ld, p, d, q, I, *ptrs(b["fit"]), **tail)
            snaps["fit"] = snapshots(b["fit"])
            r["host_fc"] = engine.forecast(self.rows, p, d, q, True, self.coef, 5)
            engine.forecast_device(b["rows"].ptr, N, T, b["rows"].ld, p, d, q, I, b["coef"].ptr, 5, b["fc"].ptr,
                                   b["fc"].ld, **tail)
            snaps["fc"] = snapshots([b["fc"]])
            r["host_dg"] = engine.diagnostics(self.rows, TH_LAG)
            engine.remove_effects_device(b["rows"].ptr, N, T, b["rows"].ld, p, d, q, I, b["coef"].ptr, b["res"].ptr,
                                         b["res"].ld, **tail)
            snaps["res"] = snapshots([b["res"]])
            r["host_gfit"] = engine.garch_fit_batch(self.grows)
            engine.diagnostics_device(b["res"].ptr, N, T, b["res"].ld, TH_LAG, *ptrs(b["dg"]), **tail)
            snaps["dg"] = snapshots(b["dg"])
            r["host_ag"] = engine.argarch_remove_effects(self.prow, self.pg)
            engine.garch_fit_batch_device(b["grows"].ptr, N, T, b["grows"].ld, *ptrs(b["gfit"]), **tail)
            snaps["gfit"] = snapshots(b["gfit"])
            engine.sample_device(b["smp"].ptr, N, T, b["smp"].ld, p, d, q, I, base, 0.05, self.seed, 0, **tail)
            snaps["smp"] = snapshots([b["smp"]])
        s.synchronize()
        outs = dict(fit=b["fit"], fc=[b["fc"]], res=[b["res"]], dg=b["dg"], gfit=b["gfit"], smp=[b["smp"]])
        for k, sn in snaps.items():
            r[k] = bodies(self.rig, s, outs[k], sn, f"thread {self.i} {k}")
        return r

    def check_alone(self, r):
        """The sequence's results, run alone, against the restatements (once per worker)."""
        p, d, q, I, _ = C1
        N, T, rows, coef = TH_N, TH_T, self.rows, self.coef
        exp = oracle_fit(rows, p, d, q, I)
        check_fit(r["host_fit"], exp, "host fit")
        check_fit(dict(zip(FIT_KEYS, r["fit"])), exp, "device fit")
        fc = np.stack([O.forecast(rows[i], p, d, q, I, coef[i], 5) for i in range(N)])
        same(r["host_fc"], fc, "host forecast")
        same(r["fc"][0], fc, "device forecast")
        diag_check(r["host_dg"], diag_ref(rows, TH_LAG), "host diagnostics")
        resid = np.stack([O.remove_time_dependent_effects(rows[i], p, d, q, I, coef[i]) for i in range(N)])
        same(r["res"][0], resid, "device residuals")
        diag_check(dict(zip(DIAG_KEYS, r["dg"])), diag_ref(resid, TH_LAG), "device diagnostics of the residuals")
        w = slice(self.off, self.off + N)
        for k, dev_out in zip(MODEL_KEYS, r["gfit"]):
            host_key = "ll" if k == "obj" else k
            same(r["host_gfit"][host_key], self.garch[k][w], f"host garch fit {k}")
            same(dev_out, self.garch[k][w], f"device garch fit {k}")
        same(r["host_ag"], self.pairs["argarch_remove"][w], "host argarch remove")
        assert np.all(np.isfinite(r["smp"][0]))


def same_results(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        xs, ys = (a[k], b[k])
        if isinstance(xs, dict):
            xs, ys = [xs[j] for j in sorted(xs)], [ys[j] for j in sorted(xs)]
        elif isinstance(xs, np.ndarray):
            xs, ys = [xs], [ys]
        for j, (x, y) in enumerate(zip(xs, ys)):
            same(y, x, f"{what} {k}[{j}]")


def test_four_threads_share_one_handle(engine, rig, handles):
    torch = rig.torch
    shared = handles()
    workers = [Worker(engine, rig, i) for i in range(4)]
    alone = []
    for w in workers:                                        # the sequence run alone, held to the restatements
        b = w.buffers()
        torch.cuda.synchronize(rig.dev)
        alone.append(w.run(shared, b))
        w.check_alone(alone[-1])
    bufs = [w.buffers() for w in workers]
    torch.cuda.synchronize(rig.dev)
    together = run_threads([lambda w=w, b=b: w.run(shared, b) for w, b in zip(workers, bufs)])
    for i, (x, y) in enumerate(zip(alone, together)):
        same_results(x, y, f"thread {i}")


def test_two_handles_two_threads(engine, rig, handles):
    # two handles on one device, a thread each: the ARIMA fit on one, the ARGARCH fixture on the other, concurrently
    torch = rig.torch
    p, d, q, I, _ = C2
    rows, decoy = _fit_rows(engine)
    N, T = rows.shape
    exp = memo("chain_fit_exp", lambda: oracle_fit(rows, p, d, q, I))
    meta, arr = load_case("argarch/argarch_T97")
    aN, aT = arr["series"].shape
    a_decoy = np.random.default_rng(11).standard_normal((aN, aT)) * 0.5
    ha, hb = handles(), handles()
    sa, sb = torch.cuda.Stream(rig.dev), torch.cuda.Stream(rig.dev)
    REPS = 3

    def arima_buffers():
        return [(In(rig.dev, rows, decoy, ld=T + 3), fit_outs(rig.dev, N, 5)) for _ in range(REPS)]

    def argarch_buffers():
        return [(In(rig.dev, arr["series"], a_decoy, ld=aT + 3), model_outs(rig.dev, aN, 5)) for _ in range(REPS)]

    def arima_job(bufs):
        out = []
        with torch.cuda.stream(sa):
            for d_rows, outs in bufs:
                d_rows.load()
                ha.fit_batch_device(d_rows.ptr, N, T, d_rows.ld, p, d, q, I, *ptrs(outs), stream=sa.cuda_stream,
                                    blocking=False)
                out.append(snapshots(outs))
        sa.synchronize()
        return [bodies(rig, sa, outs, sn, "arima thread") for (_, outs), sn in zip(bufs, out)]

    def argarch_job(bufs):
        out = []
        with torch.cuda.stream(sb):
            for d_rows, outs in bufs:
                d_rows.load()
                hb.argarch_fit_batch_device(d_rows.ptr, aN, aT, d_rows.ld, *ptrs(outs), stream=sb.cuda_stream,
                                            blocking=False)
                out.append(snapshots(outs))
        sb.synchronize()
        return [bodies(rig, sb, outs, sn, "argarch thread") for (_, outs), sn in zip(bufs, out)]

    b1, b2 = arima_buffers(), argarch_buffers()
    torch.cuda.synchronize(rig.dev)
    alone = [arima_job(b1), argarch_job(b2)]
    for got in alone[0]:
        check_fit(dict(zip(FIT_KEYS, got)), exp, "ARIMA fit alone")
    for got in alone[1]:
        for g, k in zip(got, MODEL_KEYS):
            same(g, arr[k], f"ARGARCH fit alone {k}")
    b1, b2 = arima_buffers(), argarch_buffers()
    torch.cuda.synchronize(rig.dev)
    together = run_threads([lambda: arima_job(b1), lambda: argarch_job(b2)])
    for x, y, what in zip(alone, together, ("ARIMA", "ARGARCH")):
        for rep, (gx, gy) in enumerate(zip(x, y)):
            for j, (u, v) in enumerate(zip(gx, gy)):
                same(v, u, f"{what} fit {rep} output {j}")
