"""The dead gradient pass (spark-timeseries_amd/csrc/cg_lane.hpp, CGLane's SKIPG): after a line search the reference
computes the gradient at the new point and only then, at the top of the next iteration, tests convergence on objective
values, MaxIter and MaxEval (ARIMA.scala:174-200) -- so when that test is going to stop the fit, nothing reads the
gradient and the machine posts no request for it, counting it as the reference does. tests/sim/skipg_sim.cpp runs the
machine with and without the skip on the CPU against the CPU restatement: status, coefficients, LL, n_eval and n_grad
bit for bit over the C2 fixture and the (1,0,1)+c and (5,1,5)+c orders, both smear readings, speculation off and on;
every converged fit posts exactly n_grad - 1 gradient requests; and with the machine's limits lowered, fits that stop on
MaxEval or MaxIter at the top of an iteration come out as from the machine stepped without the skip. Stand-alone
programs, once under AddressSanitizer + UBSan. The GPU side is tests/test_gpu_skipped_g.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
from conftest import load_case

SIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sim")


def _rows(order):
    p, d, q, I = order
    if order == (2, 1, 2, 1):
        return load_case("c2_212_T1024")[1]["series"][:32]
    rng = np.random.default_rng(11 * p + 3 * q + d)
    return np.stack([O.add_time_dependent_effects(rng.standard_normal(300), 1, d, 1, 1, [0.5, 0.4, 0.3])
                     for _ in range(24)])


def _run(exe_name, order, tmp_path, make_target=None):
    O.lib()                                             # the restatement's library, which the programs link
    subprocess.check_call(["make", "-s", "-C", SIM, "-f", "skipg.mk", make_target or os.path.join("_build", exe_name)])
    rows = np.ascontiguousarray(_rows(order), dtype=np.float64)
    path = os.path.join(str(tmp_path), "rows.f64")
    rows.tofile(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(SIM, "_build", exe_name), path, str(rows.shape[0]), str(rows.shape[1])] +
                       [str(v) for v in order], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "skipg OK" in r.stdout, r.stdout
    m = re.search(r"limits (\d+) (\d+) fits (\d+) ok (\d+) top_max_eval (\d+) top_max_iter (\d+) skipped (\d+) "
                  r"g_saved (\d+)", r.stdout)
    assert m, r.stdout
    names = ("max_eval", "max_iter", "fits", "ok", "top_max_eval", "top_max_iter", "skipped", "g_saved")
    out = dict(zip(names, (int(g) for g in m.groups())))
    print(order, out)
    return out, rows.shape[0]


@pytest.mark.parametrize("order", [(2, 1, 2, 1), (1, 0, 1, 1), (5, 1, 5, 1)])
def test_skip_matches_the_restatement(order, tmp_path):
    t, N = _run("skipg_sim", order, tmp_path, "skipg")
    assert (t["max_eval"], t["max_iter"]) == (10000, 10000)
    # 2 smear readings x 2 speculation policies, and no series left out (the program leaves out a series whose
    # Hannan-Rissanen init fails; these rows have none). (5,1,5)+c over these ARMA(1,1) rows: a quarter of the fits
    # converge, the others end at MaxEval
    assert t["fits"] == 4 * N
    assert t["ok"] >= N and t["skipped"] == t["g_saved"] >= t["ok"]


def test_skip_under_sanitizers(tmp_path):
    t, N = _run("skipg_sim_san", (2, 1, 2, 1), tmp_path, "skipg_san")
    assert t["fits"] == 4 * N and t["ok"] > 0


@pytest.mark.parametrize("limit", ["maxeval45", "maxeval60", "maxiter3"])
def test_stop_at_the_top_of_an_iteration(limit, tmp_path):
    # MaxEval stops a fit at the top of an iteration only when its count is exactly the limit there (the fixture has
    # such fits at 45 and at 60; most fits meet the limit inside a line search); MaxIter is tested nowhere else
    t, N = _run("skipg_sim_" + limit, (2, 1, 2, 1), tmp_path)
    assert t["fits"] == 4 * N
    assert (t["max_eval"], t["max_iter"]) == ((int(limit[7:]), 10000) if limit.startswith("maxeval") else (10000, 3))
    assert t["top_" + ("max_eval" if limit.startswith("maxeval") else "max_iter")] > 0, t
