"""The CPU side of ARGARCH, ARModel's pair and the sample recursions (no GPU):
- the reference's own known answers (GARCHSuite "standardize and filter", "fit model 2") hold on the restatement
  tests/argarch_ref.py;
- the committed fixtures regenerate bit for bit from their stored rows and satisfy the conditions the GPU tests rely on;
- the device's pass routines (csrc/model_pass.hpp), built as a stand-alone program (tests/sim/argarch_sim.cpp), equal
  the restatement bit for bit, also under the host sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import argarch_ref as R
import oracle as O
import smallfit_ref as S
from conftest import ROOT, load_case
from jvm_random import MersenneTwister

SIM_DIR = os.path.join(ROOT, "tests", "sim")


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        bad = ~((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b)))
    else:
        bad = a != b
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist(), a[bad][:5], b[bad][:5])


# ---- the reference's known answers -------------------------------------------------------------------------------
def test_garch_suite_standardize_and_filter():
    model = (40.0, .4, .2, .3, .4)
    ts = R.argarch_sample(MersenneTwister(5).gaussians(10000), *model)
    assert ts[0] == 0.0 and abs(np.mean(ts) - 40.0 / (1 - .4)) < 1.0
    standardized = R.argarch_remove(ts, *model)
    filtered = R.argarch_add(standardized, *model)
    assert max(abs(a - b) for a, b in zip(filtered, ts)) < .001


def test_garch_suite_fit_model_2():
    ts = R.suite_pattern(312)
    assert ts[:9] == [0.1, -0.2, -0.1, 0.1, 0.0, -0.01, 0.0, -0.1, 0.1] and ts[-1] == -0.1
    r = R.argarch_fit(ts)
    assert r["status"] == 0 and r["ar_status"] == 0 and all(np.isfinite(r["x"]))
    st, c, phi = O.ar_fit(ts, 1)
    assert (r["x"][0], r["x"][1]) == (c, phi[0])
    # the model's GARCH part is GARCH.fitModel of the AR residuals, and its ll their logLikelihood
    res = R.ar_remove(ts, c, [phi[0]])
    assert res[0] == ts[0] - c and res[1] == (ts[1] - c) - ts[0] * phi[0]
    assert r["obj"] == S.garch_loglik(res, *r["x"][2:])


def test_samples_and_ar_pair_edges():
    z = MersenneTwister(5).gaussians(50)
    g = R.garch_sample(z, .2, .3, .4)
    a = R.argarch_sample(z, 0.0, 0.0, .2, .3, .4)
    assert g[0] == 0.0 and g[1:] == a[1:]                    # c = phi = 0: ARGARCH's sample is GARCH's, bar -0.0 + eta
    assert g[1] == S.jsqrt(.2 + .4 * (.2 / (1 - .3 - .4)) + .3 * (S.jsqrt(.2 / (1 - .3 - .4)) * z[0]) ** 2) * z[1]
    # ARModel: for i < p only the lags that exist; remove inverts add
    coef = [.5, -.3, .2]
    y = R.ar_add(z, 1.5, coef)
    assert y[0] == 1.5 + z[0] and y[1] == (1.5 + z[1]) + y[0] * .5 and y[2] == ((1.5 + z[2]) + y[1] * .5) + y[0] * -.3
    back = R.ar_remove(y, 1.5, coef)
    assert max(abs(u - v) for u, v in zip(back, z)) < 1e-12
    assert R.ar_sample(z, 1.5, coef) == y


# ---- fixtures ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FIXTURES)
def test_goldens_regenerate(name):
    meta, arr = load_case(name)
    rows = R.fixture_rows(name)
    assert np.array_equal(rows, arr["series"], equal_nan=True) and rows.shape == (meta["N"], meta["T"])
    f = R.fit_batch(arr["series"])
    for k in ("coef", "obj", "status", "n_eval", "n_grad", "ar_status"):
        _same(f[k], arr[k], k)


def test_fixture_conditions():
    meta, arr = load_case("argarch/argarch_T97")
    assert arr["series"].shape == (130, 97) and (arr["status"] == 0).sum() >= 100
    for name in R.FIXTURES:
        meta, arr = load_case(name)
        assert (arr["status"] == R.ST_SINGULAR).sum() >= 1 and (arr["status"] == R.ST_MAX_EVAL).sum() >= 1
        assert arr["status"][5] == arr["status"][6] == R.ST_SINGULAR              # the zero row and the constant row
        failed = arr["status"] != 0
        assert np.all(np.isnan(arr["coef"][failed])) and np.all(np.isnan(arr["obj"][failed]))
        ar_failed = arr["ar_status"] != 0
        assert np.all(arr["n_eval"][ar_failed] == 0) and np.all(arr["n_grad"][ar_failed] == 0)
        assert np.all(np.isfinite(arr["coef"][~failed]))


# ---- the device's pass routines against the restatement ---------------------------------------------------------------
def _sim(tmp_path, target, mode, rows, par):
    subprocess.check_call(["make", "-s", "-C", SIM_DIR, "-f", "argarch.mk", target])
    exe = os.path.join(SIM_DIR, "_build", "argarch_sim" + ("_san" if target.endswith("san") else ""))
    rows, par = np.ascontiguousarray(rows, dtype=np.float64), np.ascontiguousarray(par, dtype=np.float64)
    (N, T), P = rows.shape, par.shape[1]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([N, T, P], np.int64).tobytes())
        f.write(rows.tobytes())
        f.write(par.tobytes())
    subprocess.check_call([exe, mode, fin, fout])
    b = open(fout, "rb").read()
    if mode != "fit":
        assert len(b) == N * T * 8
        return np.frombuffer(b, np.float64).reshape(N, T)
    assert len(b) == N * 4 * 8 + 3 * N * 4
    ints = np.frombuffer(b, np.int32, 3 * N, N * 4 * 8).reshape(3, N)
    return dict(coef=np.frombuffer(b, np.float64, N * 3).reshape(N, 3), obj=np.frombuffer(b, np.float64, N, N * 3 * 8),
                status=ints[0], n_eval=ints[1], n_grad=ints[2])


def _ar_stage(rows):
    st = np.empty(len(rows), np.int32)
    cp = np.zeros((len(rows), 2))
    for i, row in enumerate(rows):
        st[i], c, phi = O.ar_fit(row, 1)
        if st[i] == 0:
            cp[i] = (c, phi[0])
    return st, cp


@pytest.mark.parametrize("name,target,n", [("argarch/argarch_T97", "argarch", 130), ("argarch/argarch_T211", "argarch", 70),
                                           ("argarch/argarch_T97", "argarch_san", 24)])
def test_fit_pass_matches_restatement(tmp_path, name, target, n):
    meta, arr = load_case(name)
    st, cp = _ar_stage(arr["series"][:n])
    _same(st, arr["ar_status"][:n], "AR status")
    ok = st == 0
    s = _sim(tmp_path, target, "fit", arr["series"][:n][ok], cp[ok])
    _same(s["status"], arr["status"][:n][ok], "status")
    _same(s["n_eval"], arr["n_eval"][:n][ok], "n_eval")
    _same(s["n_grad"], arr["n_grad"][:n][ok], "n_grad")
    _same(s["obj"], arr["obj"][:n][ok], "obj")
    good = s["status"] == 0
    _same(s["coef"][good], arr["coef"][:n][ok][good][:, 2:], "garch coef")
    _same(cp[ok][good], arr["coef"][:n][ok][good][:, :2], "ar coef")


@pytest.mark.parametrize("T", (1, 2, 33, 97))
def test_pairs_and_samples_match_restatement(tmp_path, T):
    ref = R.pair_reference(T)
    rows, g = ref["rows"], ref["g"]
    _same(_sim(tmp_path, "argarch", "remove", rows, g), ref["argarch_remove"], "remove")
    _same(_sim(tmp_path, "argarch", "add", rows, g), ref["argarch_add"], "add")
    _same(_sim(tmp_path, "argarch", "asample", rows, g), ref["argarch_sample"], "argarch sample")
    _same(_sim(tmp_path, "argarch", "gsample", rows, g[:, 2:]), ref["garch_sample"], "garch sample")
    for p in R.AR_ORDERS:
        _same(_sim(tmp_path, "argarch", "arremove", rows, ref["ar"][p]), ref[f"ar_remove_{p}"], f"ar remove {p}")
        _same(_sim(tmp_path, "argarch", "aradd", rows, ref["ar"][p]), ref[f"ar_add_{p}"], f"ar add {p}")


def test_pairs_and_samples_under_sanitizers(tmp_path):
    # the same stand-alone program built with AddressSanitizer + UBSan (host code, its own main): clean and identical
    ref = R.pair_reference(33)
    rows, g = ref["rows"][:20], ref["g"][:20]
    _same(_sim(tmp_path, "argarch_san", "remove", rows, g), ref["argarch_remove"][:20])
    _same(_sim(tmp_path, "argarch_san", "add", rows, g), ref["argarch_add"][:20])
    _same(_sim(tmp_path, "argarch_san", "asample", rows, g), ref["argarch_sample"][:20])
    for p in (1, 20):
        _same(_sim(tmp_path, "argarch_san", "arremove", rows, ref["ar"][p][:20]), ref[f"ar_remove_{p}"][:20])
        _same(_sim(tmp_path, "argarch_san", "aradd", rows, ref["ar"][p][:20]), ref[f"ar_add_{p}"][:20])
