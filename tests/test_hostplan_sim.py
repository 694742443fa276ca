"""The host path's sizing arithmetic (spark-timeseries_amd/csrc/host_plan.hpp: chunk schedule of arima_fit_batch, the
pinned-staging layout, par_memcpy and its partition, the fit- and diag-slice rows, the extent of a strided buffer and
the entry points' buffer table against find_overlap on hand-built lists) swept on the CPU by
tests/sim/hostplan_sim.cpp: no chunk above min(host_chunk, N) (the schedule it replaced planned 16384-series tail
chunks into buffers of 8193..16383 series), plans identical to that schedule wherever it stayed in bounds, staging
regions aligned and disjoint, exact copies with untouched sentinels. Once plain, once under AddressSanitizer + UBSan
(stand-alone programs). The GPU side of the same path is tests/test_gpu_hostpath.py."""
import os
import re
import subprocess

import pytest

SIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sim")


def _run(target):
    subprocess.check_call(["make", "-s", "-C", SIM, "-f", "hostplan.mk", target])
    exe = os.path.join(SIM, "_build", "hostplan_sim" + ("_san" if target.endswith("san") else ""))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("target", ["hostplan", "hostplan_san"])
def test_host_planners(target):
    out = _run(target)
    assert "hostplan OK" in out, out
    m = re.search(r"previous schedule overruns (\d+) \(host_chunk (\d+)\.\.(\d+)\), new planner overruns (\d+)", out)
    assert m, out
    old, lo, hi, new = map(int, m.groups())
    # the defect this sweep is the failing-before proof of: 16384-series tail chunks planned for smaller buffers
    assert old > 0 and 8193 <= lo <= hi <= 16383, out
    assert new == 0, out
