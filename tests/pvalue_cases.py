"""Inputs that put the chi-squared upper tail (csrc/arima_chisq.hpp, diag_ref.chisq_upper_tail) into each of its regimes
through the two calls that reach it, shared by the CPU measurement (tests/test_diag_ref.py) and the device comparison
(tests/test_gpu_pvalue.py). No entry point takes a statistic, so the rows are built to give the statistics wanted:

  Ljung-Box (df = max_lag)   AR(1) recursions over white noise, phi from 0 (statistics around L, both sides of the
                             branch point stat = L + 2) upwards (p-values down to exact zeros)
  bptest (df = k)            white-noise residuals and factors: the statistic spreads over chi-squared(k), which
                             reaches the small-x end of the series (p close to 1)

The regimes: logGamma in closed form for L <= 16 and by Lanczos from 17; the series for stat < L + 2 and the continued
fraction from stat >= L + 2. Everything is computed once per process and left unchanged.
"""
import numpy as np

import diag_ref as R
import regress_ref as RR

SEED = 20261021
# max_lag of the Ljung-Box rows: either side of the closed-form / Lanczos switch (16 | 17), the kernel's lag groups of
# 8, and the lags the recorded tolerance was never measured at (above 40)
SMALL_L = (1, 2, 3, 4, 7, 8, 15, 16, 17, 18, 40, 64)
BIG_L = (127, 255)
MEASURED_L = (64, 127, 255)             # above the 40 lags the recorded tolerance P_TOL was measured up to
# the coverage the inputs must give on the restatement's own outputs, per L: statistics on each side of L + 2 and, up
# to L = 64, p-values in (0, 1e-3)
MIN_SIDE_SMALL, MIN_TAIL_SMALL, MIN_SIDE_BIG = 8, 8, 4

_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _ar1(phis, T):
    e = np.random.default_rng(SEED).standard_normal((len(phis), T))
    rows = np.empty_like(e)
    for i, phi in enumerate(phis):
        prev = 0.0
        for t in range(T):
            prev = phi * prev + e[i, t]
            rows[i, t] = prev
    return rows


def lb_rows(which):
    """(rows, their restated autocorrelations at the set's largest lag). "small": 128 x 300 for SMALL_L; "big":
    20 x 3072 for BIG_L (at T = 300 the statistic of 255 lags never falls below L + 2)."""
    def make():
        if which == "small":
            rows = _ar1(np.concatenate([np.zeros(32), np.linspace(0.0, 0.5, 96)]), 300)
        else:
            rows = _ar1(np.concatenate([np.zeros(12), np.linspace(0.0, 0.12, 8)]), 3072)
        return rows, [R.autocorr(r, max(SMALL_L if which == "small" else BIG_L)) for r in rows]
    return _once(("lb", which), make)


def lb_case(L):
    """(rows, acf at the set's largest lag, restated statistics, restated p-values) of max_lag L."""
    def make():
        rows, acf = lb_rows("small" if L in SMALL_L else "big")
        st = [R.lb_stat_from_acf(a[:L], rows.shape[1]) for a in acf]
        return rows, acf, np.array(st), np.array([R.chisq_upper_tail(L, s) for s in st])
    return _once(("lb_case", L), make)


def check_lb_coverage(L):
    """The condition on the inputs, asserted on the restatement before anything is compared."""
    _, _, st, pv = lb_case(L)
    side = MIN_SIDE_SMALL if L in SMALL_L else MIN_SIDE_BIG
    below, above = int(np.sum(st < L + 2)), int(np.sum(st >= L + 2))
    assert below >= side and above >= side, f"L = {L}: {below} statistics below L + 2, {above} at or above; {side} wanted"
    if L in SMALL_L:
        tail = int(np.sum((pv > 0.0) & (pv < 1e-3)))
        assert tail >= MIN_TAIL_SMALL, f"L = {L}: {tail} p-values in (0, 1e-3); {MIN_TAIL_SMALL} wanted"


def bp_case(k):
    """(residuals 128 x 64, factors 128 x 64 x k, the restatement's (status, statistic, p-value) per row)."""
    def make():
        rng = np.random.default_rng(SEED + k)
        u, f = rng.standard_normal((128, 64)), rng.standard_normal((128, 64, k))
        return u, f, [RR.bptest(u[i], f[i].T) for i in range(128)]
    return _once(("bp", k), make)


def exact_tail(L, stats):
    """The upper tail of chi-squared(L) at every statistic, from mpmath at 50 digits, rounded to double."""
    import mpmath
    with mpmath.workdps(50):
        return np.array([float(mpmath.gammainc(mpmath.mpf(L) / 2, mpmath.mpf(float(s)) / 2, mpmath.inf,
                                               regularized=True)) for s in stats])


def measured_statistics(L):
    """Where the restatement's distance from the exact value is measured for L in {64, 127, 255}: the statistics the
    device test uses, the grid L + z sqrt(2 L) for z in linspace(-6, 12, 73) (positive values only) and the three
    doubles at the branch point L + 2."""
    grid = L + np.linspace(-6.0, 12.0, 73) * np.sqrt(2.0 * L)
    edge = [np.nextafter(L + 2.0, 0.0), L + 2.0, np.nextafter(L + 2.0, np.inf)]
    st = lb_case(L)[2]
    return np.concatenate([st[np.isfinite(st) & (st > 0.0)], grid[grid > 0.0], edge])
