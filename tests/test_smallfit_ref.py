"""The CPU side of the EWMA / GARCH(1,1) fits (no GPU):
- tests/smallfit_ref.py's optimizer is pinned to the oracle (it reproduces ARIMA css-cgd fits bit for bit);
- the reference's own known answers (EWMASuite, GARCHSuite) hold on the restatement;
- the committed fixtures regenerate bit for bit and satisfy the conditions the GPU tests rely on;
- the device's optimizer state machine and pass routines (csrc/cg_small.hpp, model_pass.hpp), built as a stand-alone
  program (tests/sim/smallfit_sim.cpp), equal the restatement bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import smallfit_ref as R
from conftest import ROOT, load_case

SIM_DIR = os.path.join(ROOT, "tests", "sim")


# ---- the port is the oracle's optimizer ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,pdqi,rows", [("c1_101_T500", (1, 0, 1, 1), range(6)),
                                            ("c2_212_T1024", (2, 1, 2, 1), range(3))])
def test_port_reproduces_oracle_fits(name, pdqi, rows):
    p, d, q, I = pdqi
    meta, arr = load_case(name)
    for i in rows:
        y = O.differences_of_order_d(arr["series"][i], d)[d:]
        st, x0 = O.hannan_rissanen(y, p, q, I)
        assert st == 0
        r = R.cg_optimize(lambda x: O.loglik_css_arma(y, p, q, I, x),
                          lambda x: O.gradient_css_arma(y, p, q, I, x).tolist(), x0, 1e-7, False)
        e = O.fit(arr["series"][i], p, d, q, I)
        assert r["status"] == e["status"] == arr["status"][i]
        assert np.array_equal(r["x"], e["coef"], equal_nan=True) and np.array_equal(r["x"], arr["coef"][i], equal_nan=True)
        assert (r["n_eval"], r["n_grad"]) == (e["n_eval"], e["n_grad"]) == (arr["n_eval"][i], arr["n_grad"][i])


# ---- the reference's known answers -------------------------------------------------------------------------------
def _round2(x):
    return int(np.floor(x * 100 + 0.5)) / 100.0


def test_ewma_suite_fit_oil():
    r = R.ewma_fit(R.OIL)
    assert r["status"] == 0 and int(r["x"][0] * 100.0) == 89
    assert r["x"][0] == 0.8920138182337584 and (r["n_eval"], r["n_grad"]) == (19, 3)


def test_ewma_suite_add_and_remove():
    orig = [float(v) for v in range(1, 11)]
    for a, last in ((0.2, 6.54), (0.6, 9.33)):
        s = R.ewma_add(orig, a)
        assert s[0] == orig[0] and s[1] == a * orig[1] + (1 - a) * s[0]
        assert _round2(s[-1]) == last
    smoothed = [1.0, 1.2, 1.56, 2.05, 2.64, 3.31, 4.05, 4.84, 5.67, 6.54]
    o = R.ewma_remove(smoothed, 0.2)
    assert _round2(o[0]) == 1.0 and int(o[-1]) == 10


@pytest.fixture(scope="module")
def garch_sample():
    rng = np.random.default_rng(5)
    return R.garch_add(rng.standard_normal(2000).tolist(), .2, .3, .4)


def test_garch_suite_standardize_and_filter(garch_sample):
    std = R.garch_remove(garch_sample, .2, .3, .4)
    back = R.garch_add(std, .2, .3, .4)
    assert np.max(np.abs(np.asarray(back) - np.asarray(garch_sample))) < 1e-3


def test_garch_suite_gradient_signs_and_loglik(garch_sample):
    omega, alpha, beta = .2, .3, .4
    assert all(g < 0.0 for g in R.garch_gradient(garch_sample, omega + .1, alpha + .05, beta + .1))
    assert all(g > 0.0 for g in R.garch_gradient(garch_sample, omega - .1, alpha - .05, beta - .1))
    right = R.garch_loglik(garch_sample, .2, .3, .4)
    assert right > R.garch_loglik(garch_sample, .3, .4, .5) and right > R.garch_loglik(garch_sample, .1, .2, .3)


# ---- fixtures ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def regenerated():
    """Every golden's results recomputed by the restatement from the stored rows (once for the module)."""
    out = {}
    for name in R.FIXTURES:
        meta, arr = load_case(name)
        out[name] = (meta, arr, R.fit_batch(arr["series"], meta["model"]))
    return out


@pytest.mark.parametrize("name", R.FIXTURES)
def test_goldens_regenerate(regenerated, name):
    meta, arr, f = regenerated[name]
    model, rows = R.fixture_rows(name)
    assert model == meta["model"] and np.array_equal(rows, arr["series"], equal_nan=True)
    for k in ("coef", "obj", "status", "n_eval", "n_grad"):
        assert np.array_equal(f[k], arr[k], equal_nan=True), k


def test_fixture_conditions():
    for name in R.FIXTURES:
        meta, arr = load_case(name)
        assert arr["series"].shape == (130, meta["T"])
        assert (arr["status"] == 0).sum() >= 100
    meta, arr = load_case("smallfit/garch_T211")
    assert arr["status"][17] == R.ST_MAX_EVAL and arr["n_eval"][17] == R.MAX_EVAL      # the planted natural row
    assert np.all(np.isfinite(arr["series"][17]))
    scaled_ok = (arr["status"][3::4] == 0)
    assert np.any(arr["coef"][3::4][scaled_ok][:, 1:] < 0)                              # they leave the positive region
    failed = arr["status"] != 0
    assert np.all(np.isnan(arr["coef"][failed])) and np.all(np.isnan(arr["obj"][failed]))


@pytest.mark.parametrize("name", ["smallfit/garch_T97", "smallfit/garch_T211"])
def test_garch_fit_maximises(name):
    # no GoalType: the fit must end at a log-likelihood >= the one at the initial guess (a minimising fit fails this)
    meta, arr = load_case(name)
    n = 0
    for i in range(arr["series"].shape[0]):
        if arr["status"][i] == 0 and np.isfinite(arr["obj"][i]):
            assert arr["obj"][i] >= R.garch_loglik(arr["series"][i].tolist(), .2, .2, .2), i
            n += 1
    assert n >= 100


# ---- the device's machine against the restatement -----------------------------------------------------------------
def _sim(tmp_path, target, model, rows):
    subprocess.check_call(["make", "-s", "-C", SIM_DIR, "-f", "smallfit.mk", target])
    exe = os.path.join(SIM_DIR, "_build", "smallfit_sim" + ("_san" if target.endswith("san") else ""))
    N, T = rows.shape
    K = 1 if model == "ewma" else 3
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([N, T], np.int64).tobytes())
        f.write(np.ascontiguousarray(rows, dtype=np.float64).tobytes())
    subprocess.check_call([exe, model, fin, fout])
    b = open(fout, "rb").read()
    assert len(b) == N * (K + 1) * 8 + 3 * N * 4
    o = 0
    coef = np.frombuffer(b, np.float64, N * K, o).reshape(N, K)
    o += N * K * 8
    obj = np.frombuffer(b, np.float64, N, o)
    o += N * 8
    ints = np.frombuffer(b, np.int32, 3 * N, o).reshape(3, N)
    return dict(coef=coef, obj=obj, status=ints[0], n_eval=ints[1], n_grad=ints[2])


@pytest.mark.parametrize("name", R.FIXTURES)
def test_state_machine_matches_restatement(tmp_path, name):
    meta, arr = load_case(name)
    s = _sim(tmp_path, "smallfit", meta["model"], arr["series"])
    for k in ("coef", "obj", "status", "n_eval", "n_grad"):
        assert np.array_equal(s[k], arr[k], equal_nan=True), k


def test_state_machine_short_rows_and_oil(tmp_path):
    # T = 1 and 2 (empty and one-step recursions), and the reference's known answer through the machine
    for model, fit in (("ewma", R.ewma_fit), ("garch", R.garch_fit)):
        for T in (1, 2, 3):
            rows = np.random.default_rng(T).standard_normal((5, T))
            s = _sim(tmp_path, "smallfit", model, rows)
            for i in range(5):
                r = fit(rows[i])
                assert np.array_equal(s["coef"][i], r["x"], equal_nan=True) and s["status"][i] == r["status"]
                assert np.array_equal(s["obj"][i], r["obj"], equal_nan=True)
                assert (s["n_eval"][i], s["n_grad"][i]) == (r["n_eval"], r["n_grad"])
    s = _sim(tmp_path, "smallfit", "ewma", np.array([R.OIL]))
    assert s["coef"][0, 0] == 0.8920138182337584 and s["n_eval"][0] == 19 and s["n_grad"][0] == 3


def test_state_machine_under_sanitizers(tmp_path):
    # the same stand-alone program built with AddressSanitizer + UBSan (host code, its own main): clean and identical
    meta, arr = load_case("smallfit/ewma_T75")
    s = _sim(tmp_path, "smallfit_san", "ewma", arr["series"])
    assert np.array_equal(s["coef"], arr["coef"], equal_nan=True) and np.array_equal(s["n_eval"], arr["n_eval"])
    meta, arr = load_case("smallfit/garch_T97")
    s = _sim(tmp_path, "smallfit_san", "garch", arr["series"][:24])
    assert np.array_equal(s["coef"], arr["coef"][:24], equal_nan=True)
    assert np.array_equal(s["n_eval"], arr["n_eval"][:24])
