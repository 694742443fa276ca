"""The TimeSeriesModel pair (ARIMAModel.removeTimeDependentEffects / addTimeDependentEffects, ARIMA.scala:629-667)
through every layer that needs no GPU: the four C entry points refuse a null handle before any device work, the JNI
shim exports and forwards the two new natives, and the Scala facade declares them. The numerics are in
tests/test_gpu_effects.py."""
import ctypes
import os
import re
import subprocess

import numpy as np

import sparkts_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "jni_harness")
SO = os.path.join(HARNESS, "_build", "libjni_harness.so")
SCALA = os.path.join(ROOT, "integration", "jvm", "src", "main", "scala", "com", "cloudera", "sparkts", "models",
                     "ArimaMI355X.scala")
PREFIX = "Java_com_cloudera_sparkts_models_ArimaMI355XNative_00024_"
ARIMA_E_INVALID_ARG = -1

_vp, _i64, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32


def jni_effects():
    """The JNI harness (tests/jni_harness) with the two natives' signatures: (fn, env)."""
    subprocess.run(["make", "-s", "-C", HARNESS], check=True)      # up to date after build(): a no-op
    lib = ctypes.CDLL(SO)
    lib.fake_jni_env.restype = _vp
    fn = lambda name: getattr(lib, PREFIX + name)
    fn("create").restype = _i64
    fn("create").argtypes = [_vp, _vp, _i32]
    fn("destroy").argtypes = [_vp, _vp, _i64]
    fn("lastError").restype = ctypes.c_char_p
    fn("lastError").argtypes = [_vp, _vp, _i64]
    for name in ("removeEffectsBatch", "addEffectsBatch"):
        fn(name).argtypes = [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, ctypes.c_uint8, _vp, _vp]
    return fn, lib.fake_jni_env()


def test_entry_points_refuse_a_null_handle():
    lib = L.load()
    x, c, out = np.zeros((2, 8)), np.zeros((2, 3)), np.full((2, 8), -7.0)
    px, pc, po = (a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for a in (x, c, out))
    for name in ("arima_remove_effects_batch", "arima_add_effects_batch"):
        assert name in L.EXPORTED
        assert getattr(lib, name)(None, px, 2, 8, 1, 0, 1, 1, pc, po) == ARIMA_E_INVALID_ARG, name
    for name in ("arima_remove_effects_batch_device", "arima_add_effects_batch_device"):
        assert name in L.EXPORTED
        assert getattr(lib, name)(None, x.ctypes.data, 2, 8, 8, 1, 0, 1, 1, c.ctypes.data, out.ctypes.data, 8,
                                  None) == ARIMA_E_INVALID_ARG, name
    assert np.all(out == -7.0)


def test_jni_shim_exports_and_forwards_the_effects_natives():
    fn, env = jni_effects()
    x, c, out = np.zeros((2, 8)), np.zeros((2, 3)), np.full((2, 8), -7.0)
    for name in ("removeEffectsBatch", "addEffectsBatch"):
        assert fn(name)(env, None, 0, x.ctypes.data, 2, 8, 1, 0, 1, 1, c.ctypes.data, out.ctypes.data) == -1, name
    assert np.all(out == -7.0)


def test_scala_facade_declares_the_effects_natives():
    with open(SCALA) as f:
        src = f.read()
    natives = set(re.findall(r"@native\s+def\s+(\w+)", src))
    assert {"removeEffectsBatch", "addEffectsBatch"} <= natives
    for name in ("removeTimeDependentEffectsMany", "addTimeDependentEffectsMany"):
        assert re.search(r"def\s+" + name + r"\(model: ARIMAModel, values: Array\[Array\[Double\]\]\)", src), name
