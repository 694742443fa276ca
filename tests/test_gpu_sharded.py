"""The series-sharded path on the GPU (the unit it replaces is TimeSeriesRDD.mapSeries,
TimeSeriesRDD.scala:249-251): two ranks launched by torch.distributed.run -- a launcher process that never touches
the GPU -- each fit their contiguous shard of the same C2 batch on GPU 0 (device override) through the C ABI; the
results gathered on rank 0 must equal a single-rank fit of the whole batch bit for bit."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, out, total):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "spark-timeseries_amd"),
                                                       os.environ.get("PYTHONPATH", "")]),
               HSA_ENABLE_IPC_MODE_LEGACY="0", SPARKTS_DEVICE="0")
    args = ["-m", "sparkts_amd.shard_fit", "--total", str(total), "--T", "1024", "--out", out]
    if world == 1:
        cmd = [sys.executable] + args
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port())] + args
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out, allow_pickle=False)
    return json.loads(str(z["meta"])), {k: z[k] for k in z.files if k != "meta"}


def test_two_ranks_on_one_gpu_match_single_rank(tmp_path):
    total = 40000                              # odd split: shards of 20000 / 20000 -> also try a ragged total
    m1, one = _run(1, str(tmp_path / "one.npz"), total + 1)
    m2, two = _run(2, str(tmp_path / "two.npz"), total + 1)
    assert m1["world"] == 1 and m2["world"] == 2
    for k in one:
        a, b = one[k], two[k]
        assert a.shape == b.shape, k
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
    assert (one["status"] == 0).mean() > 0.99


def test_bench_two_ranks_on_one_gpu_checks_every_rank_against_the_oracle():
    # the multi-GPU bench line is self-checking -- every rank compares the first rows of its own
    # shard with the oracle and the verdicts meet in gloo reductions (here: 2 ranks sharing GPU 0)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--device", "0", "--series", "16384",
           "--steps", "2", "--warmup", "1", "--e2e", "1", "--cpu-seconds", "2", "--pipeline", "2"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    par = line["parity"]
    assert line["n_gpus"] == 2 and par["ranks_checked"] == 2
    assert par["oracle_rows"] >= 2 * 256 and par["bit_identical"] == par["oracle_rows"]
    assert par["every_rank_bit_identical"] and par["min_rank_fraction"] == 1.0 and par["vs_isolated"]
    assert line["cpu_baseline"] is None                     # the CPU baseline is timed at N = 1 only
    # the host-memory leg on every rank at once: both ranks' uploads, results equal to the device
    # path on every row of every rank
    e2e = line["end_to_end_host"]
    assert e2e["n_ranks"] == 2 and e2e["series"] == 2 * 16384 and e2e["rows_compared"] == 2 * 16384
    assert e2e["bit_identical_to_device_path"] and e2e["rows_identical"] == e2e["rows_compared"]
    assert e2e["value"] > 0 and e2e["GBps_in"] > 0


def test_bench_autofit_two_ranks_on_one_gpu_checks_every_rank():
    # the autoFit line on two ranks (sharing GPU 0): each rank auto-fits its own shard and compares its first rows
    # with oracle.autofit; the verdicts meet in the gloo reductions
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--device", "0", "--config", "af",
           "--series", "1024", "--steps", "1", "--warmup", "0", "--cpu-seconds", "4"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    par = line["parity"]
    assert line["n_gpus"] == 2 and par["ranks_checked"] == 2
    assert par["oracle_rows"] >= 2 and par["bit_identical"] == par["oracle_rows"] and par["every_rank_bit_identical"]
    assert line["config"]["series_total"] == 2048
