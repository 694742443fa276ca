"""The stats of the last fit as pure functions (spark-timeseries_amd/csrc/fit_stats.hpp: the counter-word names, the
one table from counter word to arima_fit_stats member, the flops formula shared by host and device, a fit's stats, the
order search's accumulation and stats, the sum over slices or chunks) compared on the CPU by tests/sim/fitstats_sim.cpp
with the three bodies of arima_runtime.cpp they replaced, field by field and bit for bit: random counter arrays, n from
0 to above 2 max(p, q) + 1, p and q in 0..5, 6, 20, every combination of the shape flags, sums of 1, 2 and 65 records
with a fault record in the first, a middle or no summand. Once plain, once under AddressSanitizer + UBSan (stand-alone
programs). The GPU side is tests/test_gpu_fit_stats.py."""
import os
import re
import subprocess

import pytest

SIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sim")


@pytest.mark.parametrize("target", ["fitstats", "fitstats_san"])
def test_fit_stats_match_the_replaced_bodies(target):
    subprocess.check_call(["make", "-s", "-C", SIM, "-f", "fitstats.mk", target])
    exe = os.path.join(SIM, "_build", "fitstats_sim" + ("_san" if target.endswith("san") else ""))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "fitstats OK" in r.stdout, r.stdout
    m = re.search(r"fits (\d+) sums (\d+) searches (\d+)", r.stdout)
    assert m and all(int(g) > 1000 for g in m.groups()), r.stdout
