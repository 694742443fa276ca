"""The layers above the ARGARCH / ARModel / sample entry points against the direct ABI calls: the Python models
(sparkts_amd.models.ARGARCH, Autoregression, GARCHModel.sample, fit_argarch_partition) and the JNI natives driven
through the fake JNIEnv of tests/jni_harness. The direct calls are pinned to the restatement by tests/test_gpu_argarch.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import argarch_ref as R
import oracle as O
from conftest import ROOT, load_case
from jvm_random import MersenneTwister

pytestmark = pytest.mark.gpu


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        bad = ~((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b)))
    else:
        bad = a != b
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist(), a[bad][:5], b[bad][:5])


def test_python_argarch_model(engine):
    from sparkts_amd import fit_argarch_partition
    from sparkts_amd.models import ARGARCH, GARCH
    meta, arr = load_case("argarch/argarch_T97")
    batch = ARGARCH.fit_models(arr["series"][:16])
    _same(batch.coefficients, arr["coef"][:16])
    _same(batch.log_likelihood, arr["obj"][:16])
    _same(batch.status, arr["status"][:16])
    _same(batch.phi, arr["coef"][:16, 1])
    for i in range(16):
        if arr["status"][i] == 0:
            one = ARGARCH.fit_model(arr["series"][i])
            _same(np.array([one.c, one.phi, one.omega, one.alpha, one.beta]), arr["coef"][i])
        else:
            with pytest.raises(ARGARCH.ARIMAFitError) as e:
                ARGARCH.fit_model(arr["series"][i])
            assert e.value.status == arr["status"][i]
    with pytest.raises(ARGARCH.SingularMatrixException):
        batch.model(5)                                        # the zero row: the AR stage's SingularMatrixException
    # GARCHSuite "standardize and filter" through the model class, on the suite's own draws
    m = ARGARCH.ARGARCHModel(40.0, .4, .2, .3, .4)
    z = MersenneTwister(5).gaussians(3000)
    ts = m.sample(z)
    _same(ts, np.array(R.argarch_sample(z, 40.0, .4, .2, .3, .4)))
    std = m.remove_time_dependent_effects(ts)
    _same(std, np.array(R.argarch_remove(ts.tolist(), 40.0, .4, .2, .3, .4)))
    dest = np.zeros(3000)
    assert m.add_time_dependent_effects(std, dest) is dest
    assert np.max(np.abs(dest - ts)) < .001
    _same(GARCH.GARCHModel(.2, .3, .4).sample(z), np.array(R.garch_sample(z, .2, .3, .4)))
    # the partition helper: records of two lengths, input order kept
    recs = [(f"k{i}", arr["series"][i][: 97 if i % 2 else 60]) for i in range(8)]
    got = list(fit_argarch_partition(recs, with_status=True))
    assert [k for k, _, _ in got] == [k for k, _ in recs]
    for i in (1, 3, 5, 7):
        _same(got[i][1], arr["coef"][i])
        assert got[i][2] == arr["status"][i]


def test_python_autoregression_model(engine):
    from sparkts_amd.models import Autoregression
    meta, arr = load_case("argarch/argarch_T97")
    rows = arr["series"][:12]
    for max_lag, no_icpt in ((1, False), (3, False), (2, True)):
        b = Autoregression.fit_models(rows, max_lag, no_icpt)
        for i in range(12):
            st, c, coef = O.ar_fit(rows[i], max_lag, no_icpt)
            assert b.status[i] == st
            if st == 0:
                _same(np.append(b.c[i], b.coefficients[i]), np.append(c, coef), f"lag {max_lag} row {i}")
                one = Autoregression.fit_model(rows[i], max_lag, no_icpt)
                _same(np.append(one.c, one.coefficients), np.append(c, coef))
            else:
                with pytest.raises(Exception):
                    b.model(i)
    # Autoregression.fitModel(ts) is ARGARCH's first stage
    first = Autoregression.fit_models(rows)
    ok = arr["status"][:12] == 0
    _same(first.c[ok], arr["coef"][:12, 0][ok])
    _same(first.coefficients[ok, 0], arr["coef"][:12, 1][ok])
    z = np.array(MersenneTwister(5).gaussians(40))
    m = Autoregression.ARModel(1.5, [.5, -.3, .2])
    y = m.sample(z)
    _same(y, np.array(R.ar_sample(z.tolist(), 1.5, [.5, -.3, .2])))
    _same(m.add_time_dependent_effects(z), y)
    _same(m.remove_time_dependent_effects(y), np.array(R.ar_remove(y.tolist(), 1.5, [.5, -.3, .2])))
    m1 = Autoregression.ARModel(.25, .9)                      # this(c, coef: Double)
    _same(m1.remove_time_dependent_effects(z), np.array(R.ar_remove(z.tolist(), .25, [.9])))


def test_jni_natives_match_direct_abi(engine):
    _vp, _i64, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    harness = os.path.join(ROOT, "tests", "jni_harness")
    subprocess.run(["make", "-s", "-C", harness], check=True)      # up to date after build(): a no-op
    lib = ctypes.CDLL(os.path.join(harness, "_build", "libjni_harness.so"))
    lib.fake_jni_env.restype = _vp
    fn = lambda name: getattr(lib, "Java_com_cloudera_sparkts_models_ArimaMI355XNative_00024_" + name)
    fn("create").restype = _i64
    fn("create").argtypes = [_vp, _vp, _i32]
    fn("destroy").argtypes = [_vp, _vp, _i64]
    fn("argarchFitBatch").argtypes = [_vp, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp]
    fx5 = ("argarchRemoveEffectsBatch", "argarchAddEffectsBatch", "argarchSampleBatch")
    for name in fx5 + ("garchSampleBatch",):
        fn(name).argtypes = [_vp, _vp, _i64, _vp, _i64, _i32, _vp, _vp]
    for name in ("arRemoveEffectsBatch", "arAddEffectsBatch"):
        fn(name).argtypes = [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp]
    env = lib.fake_jni_env()
    p = lambda a: None if a is None else a.ctypes.data
    assert fn("argarchFitBatch")(env, None, 0, None, 1, 4, None, None, None, None, None) == -1    # null handle
    h = fn("create")(env, None, 0)
    assert h != 0
    try:
        meta, arr = load_case("argarch/argarch_T97")
        N, T = 70, meta["T"]
        s = np.ascontiguousarray(arr["series"][:N])
        coef, ll = np.empty((N, 5)), np.empty(N)
        st, ne, ng = np.empty(N, np.int32), np.empty(N, np.int32), np.empty(N, np.int32)
        assert fn("argarchFitBatch")(env, None, h, p(s), N, T, p(coef), p(ll), p(st), p(ne), None) == 0
        _same(coef, arr["coef"][:N])
        _same(ll, arr["obj"][:N])
        _same(st, arr["status"][:N])
        _same(ne, arr["n_eval"][:N])
        ref = R.pair_reference(97)
        z, g = np.ascontiguousarray(ref["rows"][:N]), np.ascontiguousarray(ref["g"][:N])
        direct = dict(argarchRemoveEffectsBatch=engine.argarch_remove_effects,
                      argarchAddEffectsBatch=engine.argarch_add_effects, argarchSampleBatch=engine.argarch_sample)
        out = np.empty((N, T))
        for name in fx5:
            assert fn(name)(env, None, h, p(z), N, T, p(g), p(out)) == 0
            _same(out, direct[name](z, g), name)
            assert fn(name)(env, None, h, p(z), N, T, p(g), p(z)) == -1
        g3 = np.ascontiguousarray(g[:, 2:])
        assert fn("garchSampleBatch")(env, None, h, p(z), N, T, p(g3), p(out)) == 0
        _same(out, engine.garch_sample(z, g3), "garchSampleBatch")
        for order in (1, 20):
            a = np.ascontiguousarray(ref["ar"][order][:N])
            assert fn("arRemoveEffectsBatch")(env, None, h, p(z), N, T, order, p(a), p(out)) == 0
            _same(out, engine.ar_remove_effects(z, order, a), f"arRemove {order}")
            assert fn("arAddEffectsBatch")(env, None, h, p(z), N, T, order, p(a), p(out)) == 0
            _same(out, engine.ar_add_effects(z, order, a), f"arAdd {order}")
        assert fn("arAddEffectsBatch")(env, None, h, p(z), N, T, 0, p(g), p(out)) == -1
        assert fn("arAddEffectsBatch")(env, None, h, p(z), N, T, 21, p(g), p(out)) == -2
    finally:
        assert fn("destroy")(env, None, h) == 0
