"""The CPU restatement of the residual diagnostics (tests/diag_ref.py) against independent functions, and the layers of
the feature that need no GPU: the C entry points refuse a null handle, the JNI shim exports the two natives, the Scala
facade declares them. The device code is held to the restatement in tests/test_gpu_diag.py."""
import ctypes
import os
import re
import subprocess

import numpy as np

import diag_ref as R
import sparkts_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "jni_harness")
SO = os.path.join(HARNESS, "_build", "libjni_harness.so")
SCALA = os.path.join(ROOT, "integration", "jvm", "src", "main", "scala", "com", "cloudera", "sparkts", "models",
                     "ArimaMI355X.scala")
PREFIX = "Java_com_cloudera_sparkts_models_ArimaMI355XNative_00024_"
ARIMA_E_INVALID_ARG = -1
LB_SEED = 5          # numpy seed of the Ljung-Box property below (the reference suite's own seed is for a JVM generator)

_vp, _i64, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32


def jni_diag():
    """The JNI harness (tests/jni_harness) with the two diagnostics natives' signatures: (fn, env)."""
    subprocess.run(["make", "-s", "-C", HARNESS], check=True)      # up to date after build(): a no-op
    lib = ctypes.CDLL(SO)
    lib.fake_jni_env.restype = _vp
    fn = lambda name: getattr(lib, PREFIX + name)
    fn("create").restype = _i64
    fn("create").argtypes = [_vp, _vp, _i32]
    fn("destroy").argtypes = [_vp, _vp, _i64]
    fn("lastError").restype = ctypes.c_char_p
    fn("lastError").argtypes = [_vp, _vp, _i64]
    fn("diagnosticsBatch").argtypes = [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp]
    fn("residualDiagnosticsBatch").argtypes = [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, ctypes.c_uint8, _vp,
                                               _i32, _vp, _vp, _vp, _vp]
    return fn, lib.fake_jni_env()


def test_autocorr_restatement_against_numpy():
    rng = np.random.default_rng(20261019)
    rows = np.cumsum(rng.standard_normal((20, 100)), axis=1)
    rows[10:] = rng.standard_normal((10, 100))
    for r in rows:
        got = R.autocorr(r, 12)
        for i in range(1, 13):
            exp = np.corrcoef(r[i:], r[:-i])[0, 1]
            assert abs(got[i - 1] - exp) <= 1e-12 * abs(exp), (i, got[i - 1], exp)


def test_dwtest_restatement_against_numpy():
    rng = np.random.default_rng(3)
    r = rng.standard_normal(100)
    exp = np.sum(np.diff(r) ** 2) / np.sum(r ** 2)
    assert abs(R.dwtest(r) - exp) <= 1e-13 * exp
    assert np.isnan(R.dwtest([0.0])) and R.dwtest([2.0]) == 0.0


def test_ljung_box_property_of_the_reference_suite():
    # TimeSeriesStatisticalTestsSuite.scala:86-100: iid normals pass at lag 1, their AR(0.3) accumulation fails at lag 2
    rng = np.random.default_rng(LB_SEED)
    indep = rng.standard_normal(100)
    assert R.lbtest(indep, 1)[1] > 0.05
    dep, prior = [], 0.0
    for x in indep:
        prior = prior * 0.3 + x
        dep.append(prior)
    assert R.lbtest(dep, 2)[1] < 0.05


def test_int_product_wraps_at_46340():
    assert R.int_n_n2(46339) == 46339 * 46341 > 0
    assert R.int_n_n2(46340) == 46340 * 46342 - 2 ** 32 < 0
    acf = [0.25]
    assert R.lb_stat_from_acf(acf, 46339) > 0.0
    wrapped = R.lb_stat_from_acf(acf, 46340)
    assert wrapped < 0.0 and R.chisq_upper_tail(1, wrapped) == 1.0


def test_pvalue_restatement_against_torch_gammaincc():
    import torch
    stats = np.logspace(-3, np.log10(300), 200)
    worst = 0.0
    for lag in range(1, 41):
        ours = np.array([R.chisq_upper_tail(lag, float(s)) for s in stats])
        ind = torch.special.gammaincc(torch.full((200,), lag / 2.0, dtype=torch.float64),
                                      torch.tensor(stats / 2.0, dtype=torch.float64)).numpy()
        worst = max(worst, float(np.max(np.abs(ours - ind))))
    print(f"largest |p - gammaincc| over L = 1..40, stat in [1e-3, 300]: {worst:.3e}")
    # a cap, not a measurement: a 1e-15 series in fp64 cannot lose five more digits unless it is wrong
    assert worst <= 1e-10


def test_pvalue_restatement_against_mpmath_above_40_lags():
    # The figure above was measured up to L = 40. For the larger L the device is tested at (tests/test_gpu_pvalue.py)
    # the restatement is measured against the exact tail (mpmath at 50 digits) at that test's own statistics, a grid
    # over the bulk and both tails, and the three doubles around the branch point stat = L + 2; the device tolerance
    # P_TOL_ABOVE_40 of that module is 4 x the figure printed last.
    import pvalue_cases as PC
    worst = 0.0
    for lag in PC.MEASURED_L:
        stats = PC.measured_statistics(lag)
        dist = np.abs(np.array([R.chisq_upper_tail(lag, float(s)) for s in stats]) - PC.exact_tail(lag, stats))
        i = int(np.argmax(dist))
        print(f"L = {lag}: largest |p - exact| over {len(stats)} statistics: {dist[i]:.3e} at stat = {float(stats[i])!r}")
        worst = max(worst, float(dist[i]))
    print(f"largest |p - exact| over L in {PC.MEASURED_L}: {worst:.3e}")
    assert worst <= 1e-10                                         # the cap of the test above


def test_pvalue_header_on_the_host_equals_the_restatement_bit_for_bit():
    # csrc/arima_chisq.hpp compiled for the host goes through the same libm exp and log as the restatement, so there
    # the two agree to the bit: every L up to 41 (the closed-form logGamma up to 16, Lanczos from 17) and the larger L
    # of the device test, statistics through both branches and exactly at, just below and just above the branch point
    # stat = L + 2, and the special values. A branch taken at another point or logGamma in another form moves a
    # p-value by less than the device tolerance; it does not survive this.
    import struct
    sim = os.path.join(ROOT, "tests", "sim")
    subprocess.run(["make", "-s", "-C", sim, "-f", "chisq.mk", "chisq"], check=True)
    pairs = []
    for lag in list(range(1, 42)) + [64, 127, 255]:
        edge = [np.nextafter(lag + 2.0, 0.0), lag + 2.0, np.nextafter(lag + 2.0, np.inf)]
        special = [0.0, -1.0, 1e300, float("inf"), float("-inf"), float("nan")]
        pairs += [(lag, float(s)) for s in list(np.logspace(-3, np.log10(300 + 4 * lag), 60)) + edge + special]
    text = "".join(f"{lag} {struct.unpack('<Q', struct.pack('<d', s))[0]:x}\n" for lag, s in pairs)
    out = subprocess.run([os.path.join(sim, "_build", "chisq_host")], input=text, capture_output=True, text=True,
                         check=True, timeout=120).stdout.split()
    assert len(out) == len(pairs)
    for (lag, s), word in zip(pairs, out):
        got, ref = struct.unpack("<d", struct.pack("<Q", int(word, 16)))[0], R.chisq_upper_tail(lag, s)
        assert (got != got and ref != ref) or struct.pack("<d", got) == struct.pack("<d", ref), (lag, s, got, ref)


def test_pvalue_special_values():
    assert np.isnan(R.chisq_upper_tail(3, float("nan")))
    assert R.chisq_upper_tail(3, 0.0) == 1.0 and R.chisq_upper_tail(3, -5.0) == 1.0
    assert np.isnan(R.chisq_upper_tail(3, float("inf")))           # the library throws
    assert R.chisq_upper_tail(2, 1e300) == 0.0


def test_entry_points_refuse_a_null_handle():
    lib = L.load()
    x, c = np.zeros((2, 8)), np.zeros((2, 3))
    outs = [np.full((2, 3), -7.0)] + [np.full(2, -7.0) for _ in range(3)]
    dp = ctypes.POINTER(ctypes.c_double)
    po = [o.ctypes.data_as(dp) for o in outs]
    ro = [o.ctypes.data for o in outs]
    assert lib.arima_diagnostics_batch(None, x.ctypes.data_as(dp), 2, 8, 3, *po) == ARIMA_E_INVALID_ARG
    assert lib.arima_diagnostics_batch_device(None, x.ctypes.data, 2, 8, 8, 3, *ro, None) == ARIMA_E_INVALID_ARG
    assert lib.arima_residual_diagnostics_batch(None, x.ctypes.data_as(dp), 2, 8, 1, 0, 1, 1, c.ctypes.data_as(dp), 3,
                                                *po) == ARIMA_E_INVALID_ARG
    assert lib.arima_residual_diagnostics_batch_device(None, x.ctypes.data, 2, 8, 8, 1, 0, 1, 1, c.ctypes.data, 3, *ro,
                                                       None) == ARIMA_E_INVALID_ARG
    assert all(np.all(o == -7.0) for o in outs)


def test_jni_shim_exports_and_forwards_the_diagnostics_natives():
    fn, env = jni_diag()
    x, c = np.zeros((2, 8)), np.zeros((2, 3))
    outs = [np.full((2, 3), -7.0)] + [np.full(2, -7.0) for _ in range(3)]
    ro = [o.ctypes.data for o in outs]
    assert fn("diagnosticsBatch")(env, None, 0, x.ctypes.data, 2, 8, 3, *ro) == -1
    assert fn("residualDiagnosticsBatch")(env, None, 0, x.ctypes.data, 2, 8, 1, 0, 1, 1, c.ctypes.data, 3, *ro) == -1
    assert all(np.all(o == -7.0) for o in outs)


def test_scala_facade_declares_the_diagnostics_natives():
    with open(SCALA) as f:
        src = f.read()
    natives = set(re.findall(r"@native\s+def\s+(\w+)", src))
    assert {"diagnosticsBatch", "residualDiagnosticsBatch"} <= natives
    assert re.search(r"def\s+diagnosticsMany\(values: Array\[Array\[Double\]\], maxLag: Int\)", src)
    assert re.search(r"def\s+residualDiagnosticsMany\(model: ARIMAModel, values: Array\[Array\[Double\]\], maxLag: Int\)",
                     src)
