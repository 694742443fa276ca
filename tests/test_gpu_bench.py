"""A plain bench.py run on the GPU: the result line holds the headline and nothing of the --full measurements, and
--dump-outputs writes what the timed path computed in its last step -- checked here against a fit of the same seeded
batch through the engine of this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

N = 4097                                   # more than one block of the fit kernel, not a multiple of a wave


def test_plain_run_prints_the_headline_and_dumps_the_last_steps_outputs(tmp_path, engine):
    import torch
    out = tmp_path / "dump"
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--series", str(N), "--steps", "3",
           "--warmup", "1", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "series fitted/sec"
    assert line["higher_is_better"] is True and line["dtype"] == "f64" and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(N / (line["ms_per_step"] * 1e-3))
    assert line["config"]["series_done"] == N
    for key in ("roofline", "cpu_baseline", "parity", "default_config", "end_to_end_host"):
        assert key not in line                 # the --full measurements stay out of a plain run

    queues = os.environ.get("GPU_MAX_HW_QUEUES")       # bench.py raises it at import: keep it from later tests' children
    try:
        import bench as B
    finally:
        if queues is None:
            os.environ.pop("GPU_MAX_HW_QUEUES", None)
        else:
            os.environ["GPU_MAX_HW_QUEUES"] = queues
    p, d, q, I, T, base, jitter = B.CONFIGS["c2"]
    dev = torch.device("cuda", 0)
    series = torch.empty((N, T), dtype=torch.float64, device=dev)
    engine.sample_device(series.data_ptr(), N, T, T, p, d, q, I, base, jitter, B.SEED, 0)
    exp = engine.fit_batch(series.cpu().numpy(), p, d, q, bool(I))
    got = {k: np.load(out / f"{k}.npy") for k in ("rows", "coef", "ll", "status", "n_eval", "n_grad", "flags")}
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["rows"], np.arange(N))
    assert sum(v.nbytes for v in got.values()) <= 64_000_000
    for k, v in exp.items():
        assert got[k].shape == v.shape, k
        assert np.array_equal(got[k], v.astype(np.float64), equal_nan=True), k
