"""tests/regarima_ref.py, the CPU restatement the device Cochrane-Orcutt fits (k_cochrane_orcutt,
csrc/arima_regress.hip) are held to: the reference's own suite (RegressionARIMASuite.scala:27-67, its data under
tests/golden/regarima) at the suite's tolerances, and the edges of the procedure."""
import json
import math
import os

import numpy as np
import pytest

import regarima_ref as C
import regress_ref as R
from conftest import GOLDEN

SUITE_CASES = ["metal_vendor", "expenditure_stock"]


def suite_case(name):
    with open(os.path.join(GOLDEN, "regarima", name + ".json")) as f:
        return json.load(f)


def check_suite(case, beta, rho, n_iter):
    """The suite's assertions (beta(i) should equal(v +- tol)), and what the golden file records beyond them."""
    want = case["expected"]
    for got, v, tol in zip(beta, want["beta"], want["beta_tol"]):
        assert abs(got - v) <= tol, (got, v, tol)
    assert len(beta) == len(want["beta"])
    if "rho" in want:
        assert abs(rho - want["rho"]) <= want["rho_tol"], (rho, want["rho"])
    if "n_iter" in want:
        assert n_iter == want["n_iter"]


@pytest.mark.parametrize("name", SUITE_CASES)
def test_reference_suite(name):
    case = suite_case(name)
    fit = C.cochrane_orcutt(case["series"], [case["regressor"]], case["max_iter"])
    st, beta, rho, n_iter, _ = fit
    assert st == R.ST_OK
    check_suite(case, beta, rho, n_iter)
    if name == "metal_vendor":
        assert n_iter == 1 and C.reason(fit, 1) == C.STOP_MAX_ITER
    else:
        assert C.reason(fit, case["max_iter"]) == C.STOP_RHO == case["expected"]["stopped_by"]


# ---- the edges, as one batch of EDGE_T values and EDGE_K columns (tests/test_gpu_regarima.py runs it on the device) ----
EDGE_T, EDGE_K = 16, 2
EDGE_NAMES = ["stops-at-once", "exactly-linear", "constant-column", "nan-in-y", "nan-in-x", "inf-in-y"]
# small integers on which the QR recovers y = 2 + 3 x_0 - 4 x_1 exactly (found by search: most integer designs leave
# residuals of a few ulps, which the test below would report)
LINEAR_X = [[-3, -1, -1, -1, 2, -3, 1, 1, 3, 3, 1, 2, 0, 3, 3, 1], [-3, 2, 2, -2, 3, -3, -1, -2, 0, 2, -2, -3, -1, -2, -3, 1]]


def ar1_batch(rng, N, T, k, phis=(0.0, 0.0, 0.4, 0.8, -0.7, 0.95)):
    """y = 0.5 sum(x) + 2 + e, e AR(1) with phi drawn per series: (y (N, T), x (N, T, k))."""
    x = rng.standard_normal((N, T, k))
    phi = rng.choice(np.array(phis), size=N)
    w = rng.standard_normal((N, T))
    e = np.zeros((N, T))
    for t in range(T):
        e[:, t] = w[:, t] + (phi * e[:, t - 1] if t else 0.0)
    return 0.5 * x.sum(axis=2) + 2.0 + e, x


def edge_batch():
    """(y (N, T), x (N, T, k), {name: row}): healthy AR(1)-error series with the edge series among them, the first
    wave holding both kinds."""
    rng = np.random.default_rng(11)
    y, x = ar1_batch(rng, 70, EDGE_T, EDGE_K)
    where = dict(zip(EDGE_NAMES, (3, 9, 17, 30, 64, 66)))
    # the first white-noise draw whose plain OLS residuals pass the Durbin-Watson rule
    for _ in range(1000):
        yy = 0.5 * x[3].sum(axis=1) + 2.0 + rng.standard_normal(EDGE_T)
        if C.cochrane_orcutt(yy, x[3].T.tolist())[3] == 0:
            break
    y[3] = yy
    x[9] = np.array(LINEAR_X, dtype=np.float64).T
    y[9] = 2.0 + 3.0 * x[9, :, 0] - 4.0 * x[9, :, 1]
    x[17, :, 1] = 1.0                                  # the ones column again (EDGE_T a square: exactly eliminated)
    y[30, 5] = np.nan
    x[64, 2, 0] = np.nan
    y[66, EDGE_T - 1] = np.inf
    return y, x, where


def _nan_list(v):
    return all(math.isnan(b) for b in v)


def test_edges_of_the_procedure():
    y, x, where = edge_batch()
    fits = C.fit_batch(y, x)[4]
    st, beta, rho, n_iter, _ = fits[where["stops-at-once"]]
    i = where["stops-at-once"]
    assert (st, rho, n_iter) == (R.ST_OK, 0.0, 0) and math.copysign(1.0, rho) == 1.0
    assert beta == R.ols(y[i].tolist(), x[i].tolist(), True)[1]            # the plain OLS, untouched
    i = where["exactly-linear"]
    st, beta, rho, n_iter, _ = fits[i]
    res = R.residuals(y[i].tolist(), x[i].tolist(), beta)
    assert all(r == 0.0 for r in res) and math.isnan(C.dwtest(res))         # 0 / 0: not autocorrelated
    assert (st, rho, n_iter) == (R.ST_OK, 0.0, 0) and beta == [2.0, 3.0, -4.0]
    st, beta, rho, n_iter, _ = fits[where["constant-column"]]
    assert st == R.ST_SINGULAR and _nan_list(beta) and math.isnan(rho) and n_iter == 0
    for name in ("nan-in-y", "nan-in-x", "inf-in-y"):
        st, beta, rho, n_iter, _ = fits[where[name]]
        assert st == R.ST_OK and _nan_list(beta), name
    healthy = [f for j, f in enumerate(fits) if j not in where.values()]
    assert all(f[0] == R.ST_OK and not _nan_list(f[1]) for f in healthy)
    assert any(f[3] > 0 for f in healthy)


def shape_edge(T, k):
    rng = np.random.default_rng(100 * T + k)
    return ar1_batch(rng, 66, T, k)


@pytest.mark.parametrize("T,k,want", [(3, 2, None), (4, 3, None), (2, 2, R.ST_NOT_ENOUGH_DATA),
                                      (3, 3, R.ST_NOT_ENOUGH_DATA), (0, 1, R.ST_NO_DATA), (0, 3, R.ST_NO_DATA)])
def test_shape_edges(T, k, want):
    """T == k + 1 (want None): the first regression fits exactly; a series whose residuals pass the Durbin-Watson rule
    stops at 0, any other meets the transformed regression's k + 1 > T - 1. T == k and T == 0: the first one throws."""
    y, x = shape_edge(T, k)
    for st, beta, rho, n_iter, _ in C.fit_batch(y, x)[4]:
        assert n_iter == 0
        if st == R.ST_OK:
            assert want is None and rho == 0.0 and len(beta) == 1 + k
        else:
            assert st == (R.ST_NOT_ENOUGH_DATA if want is None else want) and _nan_list(beta) and math.isnan(rho)


def test_max_iter_below_one_is_refused():
    for m in (0, -1):
        with pytest.raises(ValueError):
            C.cochrane_orcutt([1.0, 2.0, 4.0], [[1.0, 3.0, 2.0]], m)


# ---- the parity batches of tests/test_gpu_regarima.py: every reason to stop, inside one wave ---------------------------
PARITY_SHAPES = [(24, 2, 10), (16, 1, 3), (12, 3, 10)]                      # (T, k, max_iter)
PARITY_N = 130
_PARITY = {}


def parity_case(shape):
    """One batch of PARITY_N series per shape and its restated fits, computed once; a smaller N is its leading rows."""
    if shape not in _PARITY:
        T, k, max_iter = shape
        y, x = ar1_batch(np.random.default_rng(7), PARITY_N, T, k)
        _PARITY[shape] = y, x, C.fit_batch(y, x, max_iter)
    return _PARITY[shape]


@pytest.mark.parametrize("shape", PARITY_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_parity_batches_hold_every_stopping_reason(shape):
    fits = parity_case(shape)[2][4]
    assert all(f[0] == R.ST_OK for f in fits)
    reasons = [C.reason(f, shape[2]) for f in fits]
    counts = {r: reasons.count(r) for r in (C.STOP_BEFORE_LOOP, C.STOP_DW, C.STOP_RHO, C.STOP_MAX_ITER)}
    assert all(counts.values()), counts
    assert len(set(reasons[:64])) >= 3 and len(set(reasons[64:128])) >= 3   # ... and mixed inside each full wave
