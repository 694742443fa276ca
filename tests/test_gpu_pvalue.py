"""The chi-squared upper tail on the device (csrc/arima_chisq.hpp), regime by regime, through its two device call sites:
arima_diagnostics_batch (Ljung-Box, df = max_lag) and arima_bptest_batch (df = k). The rows (tests/pvalue_cases.py) are
built to put the statistic where it is wanted; the statistic is held to the restatement bit for bit, so the p-values are
compared at identical inputs: with the restatement (tests/diag_ref.py) and with the exact tail (mpmath at 50 digits),
which an error shared by the device and the restatement cannot follow. What the rows cover is asserted on the
restatement before the device is called."""
import numpy as np
import pytest

import diag_ref as R
import pvalue_cases as PC
import regress_ref as RR
from test_gpu_diag import P_TOL, _p_close, _ref, _same

pytestmark = pytest.mark.gpu

# Above 40 lags P_TOL does not apply: it was measured for L <= 40, and the restatement itself is farther than that from
# the exact tail at L >= 127. 5.523e-14 is the largest |restated p - exact| over L in {64, 127, 255}, printed by
# tests/test_diag_ref.py::test_pvalue_restatement_against_mpmath_above_40_lags (at L = 255, stat = 264.678...; 9.603e-15
# at L = 64, 3.830e-14 at L = 127). The device may differ from the host in the last bit of exp and log, which enters
# through the same prefactor exp(-x + a log x - logGamma(a)) whose rounding sets that distance: 4 x, the margin of
# P_TOL, never above the CPU test's cap.
P_REF_DISTANCE_ABOVE_40 = 5.523e-14
P_TOL_ABOVE_40 = min(4 * P_REF_DISTANCE_ABOVE_40, 1e-10)


def _tol(L):
    return P_TOL if L <= 40 else P_TOL_ABOVE_40


def _check_p(got, ref, exact, L, what):
    """The device p-values against the restatement's and against the exact ones, every figure printed first."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaNs in other places"
    ok = ~np.isnan(ref)
    d_ref, d_exact = np.abs(got[ok] - ref[ok]), np.abs(got[ok] - exact[ok])
    i, j = int(np.argmax(d_ref)), int(np.argmax(d_exact))
    print(f"\n{what}: largest |device - restatement| {d_ref[i]:.3e} (row {i}), |device - exact| {d_exact[j]:.3e} "
          f"(row {j}); tolerance {_tol(L):.3e}")
    assert d_ref[i] <= _tol(L), f"{what}: {d_ref[i]:.3e} from the restatement at row {i}"
    assert d_exact[j] <= _tol(L), f"{what}: {d_exact[j]:.3e} from the exact tail at row {j}"
    assert np.all((got[ok] >= 0.0) & (got[ok] <= 1.0)), f"{what}: a p-value outside [0, 1]"


# ---- 1. Ljung-Box: the series and the continued fraction, the closed-form logGamma and Lanczos --------------------------
@pytest.mark.parametrize("L", PC.SMALL_L + PC.BIG_L)
def test_lb_pvalue_regimes(engine, L):
    PC.check_lb_coverage(L)
    rows, acf, st, pv = PC.lb_case(L)
    got = engine.diagnostics(rows, L, ("lb_stat", "lb_pvalue"))
    assert _same(got["lb_stat"], st), f"L = {L}: the statistic"
    what = (f"L = {L}: {int(np.sum(st < L + 2))} statistics below L + 2, {int(np.sum(st >= L + 2))} from it, "
            f"{int(np.sum((pv > 0) & (pv < 1e-3)))} p-values in (0, 1e-3), {int(np.sum(pv == 0))} zeros")
    _check_p(got["lb_pvalue"], pv, PC.exact_tail(L, st), L, what)
    if L <= 40:
        assert _p_close(got["lb_pvalue"], pv)                      # the module's own comparison, unchanged


# ---- 2. bptest: the small-x end of the series ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_bp_pvalue_small_statistics(engine, k):
    u, f, ref = PC.bp_case(k)
    st, pv = np.array([r[1] for r in ref]), np.array([r[2] for r in ref])
    assert all(r[0] == RR.ST_OK for r in ref)
    # chi-squared(k) over 128 rows: about 13 p-values above 0.9 and 11 (k = 1) or 17 (k = 2) statistics from k + 2
    near_one, cf = int(np.sum(pv > 0.9)), int(np.sum(st >= k + 2))
    assert near_one >= 4 and cf >= 4 and int(np.sum((st > 0) & (st < k + 2))) >= 64, (k, near_one, cf)
    got = engine.bptest(u, f)
    assert np.array_equal(got["status"], [r[0] for r in ref]) and _same(got["stat"], st), f"k = {k}: the statistic"
    pos = st > 0.0                                                 # a negative R squared: p = 1.0, no tail to evaluate
    exact = np.ones_like(st)
    exact[pos] = PC.exact_tail(k, st[pos])
    _check_p(got["pvalue"], pv, exact, k, f"bptest k = {k}: {near_one} p-values above 0.9, smallest statistic "
                                           f"{st[pos].min():.3e}")


# ---- 3. special statistics -----------------------------------------------------------------------------------------------
def test_minus_infinite_statistic_has_p_one(engine):
    # a constant non-zero u: u^2 is constant, TSS = 0, RSS > 0 by rounding, R^2 = 1 - RSS / 0 = -inf
    rng = np.random.default_rng(3)
    u, f = rng.standard_normal((66, 20)), rng.standard_normal((66, 20, 2))
    u[[0, 63, 64, 65]] = 3.25
    ref = [RR.bptest(u[i], f[i].T) for i in range(66)]
    for i in (0, 63, 64, 65):
        assert ref[i] == (RR.ST_OK, -np.inf, 1.0), (i, ref[i])
    got = engine.bptest(u, f)
    assert np.array_equal(got["status"], [r[0] for r in ref]) and _same(got["stat"], [r[1] for r in ref])
    assert _p_close(got["pvalue"], [r[2] for r in ref])
    assert np.all(got["stat"][[0, 63, 64, 65]] == -np.inf) and np.all(got["pvalue"][[0, 63, 64, 65]] == 1.0)


def test_infinite_statistic_has_p_nan(engine):
    # Lag 1: the deviations of ts[1:] are about 1e-170, so their squares underflow and v1 = 0, while ts[0] = 1e150 gives
    # ts[:-1] a deviation large enough for a non-zero covariance: the correlation is cov / 0 = +-inf, the Ljung-Box sum
    # +inf, and the continued fraction NaN (the library throws there; the header's rule for a batch is NaN).
    T = 24
    rows = np.random.default_rng(4).standard_normal((3, T))
    rows[1] = 1e-170 * np.where(np.arange(T) % 2 == 0, 1.0, -1.0)
    rows[1, 0] = 1e150
    for L in (1, 9):
        acf, dw, st, pv = _ref(rows, L)
        assert np.isinf(acf[1, 0]) and st[1] == np.inf and np.isnan(pv[1]), (L, acf[1], st[1], pv[1])
        assert np.all(np.isfinite(st[[0, 2]])) and not np.any(np.isnan(pv[[0, 2]]))
        assert st[1] == R.lbtest(rows[1], L)[0]
        got = engine.diagnostics(rows, L)
        assert _same(got["acf"], acf) and _same(got["dw"], dw) and _same(got["lb_stat"], st), f"L = {L}"
        assert _p_close(got["lb_pvalue"], pv) and np.isnan(got["lb_pvalue"][1]), f"L = {L}"
