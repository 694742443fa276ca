"""Inputs of tests/test_gpu_generic_edges.py (the runtime-order path, arima_generic.hip, at its edges) and the
conditions that keep those tests meaningful and short, checked here on the CPU with the oracle alone.

Every builder is a plain function of fixed seeds; every oracle result is computed once per process (lru_cache) and
shared by the CPU test that pins its conditions and the GPU test that compares the library with it. The arrays the
cached functions return are read-only: no test changes them.
"""
import functools

import numpy as np
import pytest

import oracle as O

ST_OK, ST_MAX_EVAL, ST_SINGULAR, ST_NOT_ENOUGH_DATA, ST_NO_DATA, ST_SERIES_TOO_SHORT = 0, 1, 4, 5, 6, 10
SHAPE_STATUSES = (ST_SERIES_TOO_SHORT, ST_NO_DATA, ST_NOT_ENOUGH_DATA)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _outside_batch(poly):
    """O._all_roots_outside_unit_circle over the rows of poly (N x (n + 1), constant term first): one stacked
    eigenvalue call for the rows of full degree, the oracle's own function for the rest (a non-finite coefficient, a
    zero leading one)."""
    N, n = poly.shape[0], poly.shape[1] - 1
    plain = np.isfinite(poly).all(axis=1) & (poly[:, n] != 0.0)
    out = np.zeros(N, dtype=bool)
    if plain.any():
        c = poly[plain]
        comp = np.zeros((len(c), n, n))
        comp[:, n - 1, :] = -c[:, :n] / c[:, n:n + 1]
        if n > 1:
            comp[:, :n - 1, 1:] = np.eye(n - 1)
        out[plain] = ~np.any(np.abs(np.linalg.eigvals(comp)) <= 1.0, axis=1)
    for i in np.flatnonzero(~plain):
        out[i] = O._all_roots_outside_unit_circle(poly[i])
    return out


def flags_batch(coef, p, q, I):
    """O.model_flags for every row of coef (the same companion matrices, stacked: a batch of 262 209 fits has its
    flags in a second instead of a quarter of a minute)."""
    coef = np.asarray(coef, dtype=np.float64).reshape(-1, p + q + I)
    N = len(coef)
    st = _outside_batch(np.concatenate([np.ones((N, 1)), -coef[:, I:I + p]], axis=1)) if p else np.ones(N, dtype=bool)
    inv = _outside_batch(np.concatenate([np.ones((N, 1)), coef[:, I + p:]], axis=1)) if q else np.ones(N, dtype=bool)
    return (st.astype(np.uint8) | (inv.astype(np.uint8) << 1)).astype(np.uint8)


def test_flags_batch_is_the_oracles_model_flags():
    rng = np.random.default_rng(11)
    for p, q, I in [(0, 6, 0), (6, 0, 1), (7, 2, 1), (20, 20, 1), (1, 1, 0)]:
        c = rng.uniform(-2.0, 2.0, (300, p + q + I)) / max(p, q)
        c[0, -1] = 0.0                                       # the degree drops
        c[1, I] = np.nan
        c[2, -1] = np.inf
        want = np.array([O.model_flags(ci, p, q, I) for ci in c], dtype=np.uint8)
        assert np.array_equal(flags_batch(c, p, q, I), want), (p, q, I)
        assert len(np.unique(want)) >= 2


def expect(s, p, d, q, I, method=0, smear=O.DEFAULT_SMEAR):
    """O.fit_batch in the layout check_fit (tests/test_gpu_parity.py) compares with Engine.fit_batch's."""
    st, coef, ll, cnt = O.fit_batch(s, p, d, q, I, method=method, smear=smear)
    flags = np.where(st == 0, flags_batch(coef, p, q, I), 0).astype(np.uint8)
    return dict(status=_frozen(st), coef=_frozen(coef), ll=_frozen(ll), n_eval=_frozen(cnt[:, 0]),
                n_grad=_frozen(cnt[:, 1]), flags=_frozen(flags))


# ---- the shape checks restated (ARIMA.scala:216-242 hannanRissanenInit, Autoregression.scala:38-53 and commons
# validateSampleData): what a fit of n differenced values reports before it reads one ------------------------------
def ols_check(rows, ncx, intercept):
    if rows <= 0:
        return ST_NO_DATA
    if ncx + 1 > rows:
        return ST_NOT_ENOUGH_DATA
    if not intercept and ncx == 0:
        return ST_NO_DATA
    return ST_OK


def shape_status(n, p, q, I):
    if p > 0 and q == 0:                                   # the AR-only shortcut (ARIMA.scala:90-96)
        return ST_SERIES_TOO_SHORT if n - p < 0 else ols_check(n - p, p, I)
    M = max(p, q)
    m = M + 1
    if n - m < 0:
        return ST_SERIES_TOO_SHORT
    st = ols_check(n - m, m, 1)
    if st != ST_OK:
        return st
    nt = n - m
    if nt - p < 0 or nt - q < 0:
        return ST_SERIES_TOO_SHORT
    return ols_check(max(nt - M, 0), p + q, I)


# ---- 1. the length sweep ------------------------------------------------------------------------------------------
SWEEP_ORDERS = [(7, 1, 2, 1), (6, 0, 0, 0), (6, 0, 0, 1), (0, 0, 6, 0), (5, 0, 6, 1), (6, 0, 5, 0), (20, 1, 0, 0),
                (20, 0, 20, 1)]
SWEEP_N = 3
# the first T whose fit gets past the shape checks: T - d = 2M + p + q + 2 for the two regressions of
# Hannan-Rissanen (M + 1 + (M + 1) + 1 rows for the AR(M + 1) stage never binds later than the second regression's
# p + q + 1), T - d = 2p + 1 for the AR shortcut
SWEEP_FIRST_PASS = {(7, 1, 2, 1): 26, (6, 0, 0, 0): 13, (6, 0, 0, 1): 13, (0, 0, 6, 0): 20, (5, 0, 6, 1): 25,
                    (6, 0, 5, 0): 25, (20, 1, 0, 0): 42, (20, 0, 20, 1): 82}


def order_id(o):
    return "".join(str(v) for v in o[:3]) + ("c" if o[3] else "") if max(o[:3]) < 10 else \
        "_".join(str(v) for v in o[:3]) + ("c" if o[3] else "")


def sweep_lengths(order):
    """Every T from 0 to 2M + p + q + d + 6; ARIMA(20,0,20)+c stops at 84, three lengths past its threshold (its
    passing fits run to the evaluation cap at K = 41)."""
    p, d, q, I = order
    top = 2 * max(p, q) + p + q + d + 6
    if order == (20, 0, 20, 1):
        top = 84
    return list(range(0, top + 1))


@functools.lru_cache(maxsize=None)
def sweep_rows(order):
    """SWEEP_N random walks; the fit at length T reads their first T values."""
    p, d, q, I = order
    rng = np.random.default_rng(9000 + 100 * p + 10 * q + 2 * d + I)
    return _frozen(rng.standard_normal((SWEEP_N, sweep_lengths(order)[-1])).cumsum(axis=1))


@functools.lru_cache(maxsize=None)
def sweep_expect(order):
    """{T: expect(rows[:, :T])}"""
    p, d, q, I = order
    rows = sweep_rows(order)
    return {T: expect(rows[:, :T], p, d, q, I) for T in sweep_lengths(order)}


@pytest.mark.parametrize("order", SWEEP_ORDERS, ids=order_id)
def test_sweep_crosses_every_shape_status(order):
    p, d, q, I = order
    exp = sweep_expect(order)
    first = SWEEP_FIRST_PASS[order]
    lengths = sweep_lengths(order)
    assert lengths[0] == 0 and first + 2 <= lengths[-1]
    seen = set()
    for T in lengths:
        st = exp[T]["status"]
        want = shape_status(max(T - d, 0), p, q, I)
        if T < first:
            assert want in SHAPE_STATUSES and np.all(st == want), (T, st, want)
        else:
            assert want == ST_OK and not np.isin(st, SHAPE_STATUSES).any(), (T, st)
        seen.update(int(s) for s in st)
    assert set(SHAPE_STATUSES) <= seen, seen
    # at the first passing length the last regression has p + q + 1 rows: with an intercept it is square (rows ==
    # columns, gen_ols' last stage runs no row loop), without one it has a single row to spare
    n = first - d
    rows = n - p if q == 0 else n - (max(p, q) + 1) - max(p, q)
    assert rows == p + q + 1 and (rows == p + q + I) == bool(I)
    at_first = exp[first]["status"]
    assert np.isin(at_first, (ST_OK, ST_MAX_EVAL, ST_SINGULAR)).all(), at_first
    past = np.concatenate([exp[T]["status"] for T in lengths if T >= first])
    n_max_eval = int((past == ST_MAX_EVAL).sum())
    if order == (20, 0, 20, 1):
        assert len(past) == 3 * SWEEP_N                      # T = 82..84 at N = 3 and nothing larger
    else:
        assert (past == ST_OK).any(), past                   # coefficients and log-likelihoods do get compared
    # rows at the evaluation cap cost 10 000 passes each on one lane: few, and only at these short lengths
    assert n_max_eval <= 3 * SWEEP_N, (order, n_max_eval)


# ---- 2. the grid stride -------------------------------------------------------------------------------------------
GEN_GRID_MAX, GEN_BLOCK = 4096, 64                           # kGenGridMax workgroups of 64 lanes (arima_generic.hip)
STRIDE_N = GEN_GRID_MAX * GEN_BLOCK + 65
STRIDE_T = 32
STRIDE_ORDERS = [(0, 0, 6, 0), (6, 0, 0, 1)]


@functools.lru_cache(maxsize=None)
def stride_rows():
    return _frozen(np.random.default_rng(4242).standard_normal((STRIDE_N, STRIDE_T)))


@functools.lru_cache(maxsize=None)
def stride_expect(order):
    p, d, q, I = order
    return expect(stride_rows(), p, d, q, I)


def test_stride_batch_is_past_the_grid_and_mostly_converges():
    assert STRIDE_N > GEN_GRID_MAX * GEN_BLOCK
    rows = stride_rows()
    # distinct rows: a lane that repeats or skips a series cannot land on an equal neighbour
    assert len(np.unique(rows[:, 0])) == STRIDE_N
    ma = stride_expect((0, 0, 6, 0))
    assert (ma["status"] == ST_MAX_EVAL).mean() <= 0.005, (ma["status"] == ST_MAX_EVAL).sum()
    assert (ma["status"] == ST_OK).mean() >= 0.98
    # the rows only the second trip of a lane reaches hold fits of their own, not statuses alone
    tail = slice(GEN_GRID_MAX * GEN_BLOCK, STRIDE_N)
    assert (ma["status"][tail] == ST_OK).sum() >= 60 and ma["n_eval"][tail].min() > 0
    ar = stride_expect((6, 0, 0, 1))
    assert np.all(ar["status"] == ST_OK) and np.all(ar["n_eval"] == 0)


# ---- 3. forecast slices -------------------------------------------------------------------------------------------
def gen_forecast_ws(T, d, M, n_future):
    """Doubles of workspace per series of the runtime-order forecast (gen_lane.hpp GenFcLayout<false>)."""
    n = T - d
    hist_len = M + n
    fl = n_future + M
    return 2 * (T + 1) + 2 * (hist_len + 1) + (fl + 1) + (d + 1) * T + 2 * (d + n_future + 1)


def forecast_slice(N, T, p, d, q, n_future):
    """Series per launch of the workspace kernel (arima_runtime.cpp forecast_slices): max(1, min(N, 2^27 / w))."""
    w = gen_forecast_ws(T, d, max(p, q), n_future)
    return max(1, min(N, (1 << 27) // max(w, 1)))


SLICE_ORDER, SLICE_T, SLICE_NF = (6, 16, 1, 1), 512, 5
SLICE_N = (1 << 27) // gen_forecast_ws(SLICE_T, 16, 6, SLICE_NF) + 65


@functools.lru_cache(maxsize=None)
def slice_inputs():
    rng = np.random.default_rng(31337)
    p, d, q, I = SLICE_ORDER
    s = rng.standard_normal((SLICE_N, SLICE_T)).cumsum(axis=1) + 3.0
    coef = rng.uniform(-0.3, 0.3, (SLICE_N, p + q + I))
    return _frozen(s), _frozen(coef)


@functools.lru_cache(maxsize=None)
def slice_expect():
    p, d, q, I = SLICE_ORDER
    s, coef = slice_inputs()
    return _frozen(np.stack([O.forecast(s[i], p, d, q, I, coef[i], SLICE_NF) for i in range(SLICE_N)]))


def test_forecast_batch_crosses_its_slice():
    p, d, q, I = SLICE_ORDER
    assert gen_forecast_ws(SLICE_T, d, max(p, q), SLICE_NF) == 10792
    sl = forecast_slice(SLICE_N, SLICE_T, p, d, q, SLICE_NF)
    assert sl == 12436 and sl < SLICE_N < 2 * sl
    exp = slice_expect()
    assert exp.shape == (SLICE_N, SLICE_T + SLICE_NF) and np.isfinite(exp).all()
    # rows on the two sides of the boundary differ everywhere: an offset dropped from one pointer shows
    assert not np.any(exp[sl:] == exp[:SLICE_N - sl])


# ---- 4. forecast short and extreme shapes -------------------------------------------------------------------------
SHORT_ORDERS = [(7, 1, 2, 1), (0, 0, 9, 1), (1, 12, 1, 0), (6, 16, 6, 1)]
SHORT_NF = (0, 1, 3)
SHORT_N = (1, 65)


def short_lengths(order):
    p, d, q, I = order
    M = max(p, q)
    return sorted({d, d + 1, d + 2, d + M - 1, d + M, d + M + 1})


@functools.lru_cache(maxsize=None)
def short_inputs(order):
    p, d, q, I = order
    rng = np.random.default_rng(700 + 31 * p + 7 * d + q)
    N, T = max(SHORT_N), short_lengths(order)[-1]
    return _frozen(rng.standard_normal((N, T)).cumsum(axis=1) + 3.0), _frozen(rng.uniform(-0.3, 0.3, (N, p + q + I)))


@functools.lru_cache(maxsize=None)
def short_expect(order):
    """{(T, n_future): N x (T + n_future)} for the largest N; a smaller batch is its first rows."""
    p, d, q, I = order
    s, coef = short_inputs(order)
    return {(T, nf): _frozen(np.stack([O.forecast(s[i, :T], p, d, q, I, coef[i], nf) for i in range(len(s))])
                             .reshape(len(s), T + nf))
            for T in short_lengths(order) for nf in SHORT_NF}


@pytest.mark.parametrize("order", SHORT_ORDERS, ids=order_id)
def test_short_forecast_shapes_are_defined(order):
    p, d, q, I = order
    Ts = short_lengths(order)
    assert Ts[0] == d and all(T >= d for T in Ts)
    if d == 0:
        assert 0 in Ts
    exp = short_expect(order)
    for (T, nf), e in exp.items():
        assert e.shape == (max(SHORT_N), T + nf)
        assert np.isfinite(e).all(), (order, T, nf)


# ---- 5. maximum orders and the dispatch boundary ------------------------------------------------------------------
BLOCK_PQ = [(20, 20), (20, 6), (6, 20)]
BLOCK_N, BLOCK_T = 40, 97


@functools.lru_cache(maxsize=None)
def block_inputs(pq):
    """N x T rows and, per intercept, (coefficients in +-0.3 / order, wide coefficients in +-4 / order). The first
    are models well inside the unit circle, for the gradient and the log-likelihood; the wide ones are for the flags
    alone, where both outcomes must occur."""
    p, q = pq
    rng = np.random.default_rng(p * 31 + q)
    y = rng.standard_normal((BLOCK_N, BLOCK_T))
    coefs = {}
    for I in (0, 1):
        c, w = (np.concatenate([rng.uniform(-a, a, (BLOCK_N, I)), rng.uniform(-a, a, (BLOCK_N, p)) / p,
                                rng.uniform(-a, a, (BLOCK_N, q)) / q], axis=1) for a in (0.3, 4.0))
        coefs[I] = (_frozen(c), _frozen(w))
    return _frozen(y), coefs


@functools.lru_cache(maxsize=None)
def block_expect(pq):
    p, q = pq
    y, coefs = block_inputs(pq)
    out = {}
    for I in (0, 1):
        c, w = coefs[I]
        out[I] = dict(
            grad={sm: _frozen(np.stack([O.gradient_css_arma(y[i], p, q, I, c[i], sm) for i in range(BLOCK_N)]))
                  for sm in (0, 1)},
            ll=_frozen(np.array([O.loglik_css(y[i], p, 0, q, I, c[i]) for i in range(BLOCK_N)])),
            flags=_frozen(np.array([O.model_flags(ci, p, q, I) for ci in c], dtype=np.uint8)),
            wide_flags=_frozen(np.array([O.model_flags(wi, p, q, I) for wi in w], dtype=np.uint8)))
    return out


@pytest.mark.parametrize("pq", BLOCK_PQ, ids=lambda pq: f"{pq[0]}_{pq[1]}")
def test_block_inputs_are_finite_and_mixed(pq):
    p, q = pq
    _, coefs = block_inputs(pq)
    exp = block_expect(pq)
    for I in (0, 1):
        c, w = coefs[I]
        assert c.shape == w.shape == (BLOCK_N, p + q + I)
        assert np.abs(c[:, I:I + p]).max() <= 0.3 / p and np.abs(c[:, I + p:]).max() <= 0.3 / q
        assert np.isfinite(exp[I]["grad"][0]).all() and np.isfinite(exp[I]["grad"][1]).all()
        assert np.isfinite(exp[I]["ll"]).all()
        assert not np.array_equal(exp[I]["grad"][0], exp[I]["grad"][1])      # the two readings of :526 differ
        assert np.all(exp[I]["flags"] == 3)
        # stationary or not, invertible or not: every bit takes both values among the wide models
        wf = exp[I]["wide_flags"]
        assert (wf & 1).any() and not (wf & 1).all() and (wf & 2).any() and not (wf & 2).all(), wf


HR_MAX = (20, 20, 1)
HR_MAX_N, HR_MAX_T = 8, 200


HR_MAX_SQUARE = 82                                           # its second regression: 41 rows, 41 columns


@functools.lru_cache(maxsize=None)
def hr_max_inputs():
    """ARMA(1,1) rows of HR_MAX_T values, and the sweep's rows at the square length and one past it (the fits
    there end at the evaluation cap, which would hide a wrong start)."""
    rng = np.random.default_rng(2020)
    long_rows = np.stack([O.add_time_dependent_effects(rng.standard_normal(HR_MAX_T), 1, 0, 1, 1, [0.5, 0.4, 0.3])
                          for _ in range(HR_MAX_N)])
    walks = sweep_rows((20, 0, 20, 1))
    return _frozen(long_rows), _frozen(walks[:, :HR_MAX_SQUARE]), _frozen(walks[:, :HR_MAX_SQUARE + 1])


@functools.lru_cache(maxsize=None)
def hr_max_expect():
    out = []
    for y in hr_max_inputs():
        r = [O.hannan_rissanen(row, *HR_MAX) for row in y]
        out.append((_frozen(np.array([st for st, _ in r], dtype=np.int32)), _frozen(np.stack([ini for _, ini in r]))))
    return out


def test_hr_at_the_maximum_order_converges_on_cpu():
    assert HR_MAX_SQUARE == SWEEP_FIRST_PASS[(20, 0, 20, 1)]
    assert shape_status(HR_MAX_SQUARE - 1, 20, 20, 1) == ST_NOT_ENOUGH_DATA
    for y, (st, ini) in zip(hr_max_inputs(), hr_max_expect()):
        assert np.all(st == ST_OK) and np.isfinite(ini).all() and ini.shape == (len(y), 41)


# (p, d, q, I, smear): the maximum orders, then the dispatch boundary (5 | 6) and the smear = 0 fits
FIT_CASES = [(20, 1, 0, 0, 1), (0, 0, 20, 1, 1), (20, 0, 6, 0, 1), (6, 0, 20, 1, 0),
             (5, 1, 6, 1, 1), (6, 1, 5, 0, 1), (7, 1, 2, 1, 0), (0, 1, 8, 0, 0)]
FIT_N, FIT_T, FIT_POOL = 16, 160, 40
FIT_MAX_EVAL_ROWS, FIT_OK_EVAL_CAP, FIT_MIN_OK = 4, 2500, 4


def fit_case_id(c):
    return order_id(c[:4]) + f"_s{c[4]}"


@functools.lru_cache(maxsize=None)
def fit_case(case):
    """(rows, expect): the first FIT_N rows of a white-noise pool (integrated once for d = 1) that keep the case
    short on one lane -- no converged row above FIT_OK_EVAL_CAP oracle evaluations and at most FIT_MAX_EVAL_ROWS rows
    that run to the evaluation cap. The choice reads the oracle alone."""
    p, d, q, I, smear = case
    rng = np.random.default_rng(5000 + 97 * p + 13 * q + 3 * d + I + 7 * smear)
    pool = rng.standard_normal((FIT_POOL, FIT_T))
    for _ in range(d):
        pool = pool.cumsum(axis=1)
    e = expect(pool, p, d, q, I, smear=smear)
    keep, capped = [], 0
    for i in range(FIT_POOL):
        st = e["status"][i]
        if st == ST_OK and e["n_eval"][i] > FIT_OK_EVAL_CAP:
            continue
        if st == ST_MAX_EVAL:
            if capped == FIT_MAX_EVAL_ROWS:
                continue
            capped += 1
        keep.append(i)
        if len(keep) == FIT_N:
            break
    keep = np.array(keep)
    return _frozen(pool[keep]), {k: _frozen(v[keep]) for k, v in e.items()}


@pytest.mark.parametrize("case", FIT_CASES, ids=fit_case_id)
def test_fit_case_is_short_and_converges(case):
    rows, e = fit_case(case)
    assert rows.shape == (FIT_N, FIT_T) and FIT_T <= 300
    ok = e["status"] == ST_OK
    assert ok.sum() >= FIT_MIN_OK, e["status"]
    assert (e["status"] == ST_MAX_EVAL).sum() <= FIT_MAX_EVAL_ROWS, e["status"]
    assert e["n_eval"][ok].max() <= FIT_OK_EVAL_CAP, e["n_eval"]
    p, d, q, I, smear = case
    if not (p > 0 and q == 0):
        assert e["n_eval"][ok].min() > 0                      # the optimizer ran (the AR shortcut counts nothing)
        # the conjugate-gradient restart (iter % n, n = the parameter count): some row iterates past it
        assert e["n_grad"].max() > p + q + I, e["n_grad"]


# ---- 6. special values --------------------------------------------------------------------------------------------
SPECIAL_ORDERS = [(7, 1, 2, 1), (9, 0, 0, 1)]
SPECIAL_T = 120
SPECIAL_ROWS = ("clean", "nan_mid", "inf_first", "constant", "nan_last", "ramp", "clean", "clean")
# a non-finite value sends the optimizer to the evaluation cap and passes through the AR shortcut's regression (a
# normal return at a NaN model); a constant row and a ramp are singular designs. The seeds give clean rows that
# converge at both ends of the batch (and one, for ARIMA(7,1,2)+c, that runs to the cap)
SPECIAL_STATUS = {(7, 1, 2, 1): [0, 1, 1, 4, 1, 4, 1, 0], (9, 0, 0, 1): [0, 0, 0, 4, 0, 4, 0, 0]}
SPECIAL_SEED = {(7, 1, 2, 1): 611, (9, 0, 0, 1): 615}
SPECIAL_CLEAN = (0, 6, 7)


@functools.lru_cache(maxsize=None)
def special_rows(order):
    p, d, q, I = order
    rng = np.random.default_rng(SPECIAL_SEED[order])
    base = {(7, 1, 2, 1): [0.2, 0.3, -0.1, 0.1, 0.05, -0.05, 0.04, 0.02, 0.3, 0.1],
            (9, 0, 0, 1): [1.0, 0.3, -0.1, 0.1, 0.05, -0.05, 0.04, 0.02, -0.02, 0.01]}[order]
    rows = np.stack([O.add_time_dependent_effects(rng.standard_normal(SPECIAL_T), p, d, q, I, base)
                     for _ in SPECIAL_ROWS])
    rows[1, SPECIAL_T // 2] = np.nan
    rows[2, 0] = np.inf
    rows[3, :] = 2.5
    rows[4, -1] = np.nan
    rows[5, :] = 1.0 + 0.25 * np.arange(SPECIAL_T)
    return _frozen(rows)


@functools.lru_cache(maxsize=None)
def special_expect(order):
    return expect(special_rows(order), *order)


@pytest.mark.parametrize("order", SPECIAL_ORDERS, ids=order_id)
def test_special_rows_give_their_statuses(order):
    e = special_expect(order)
    assert [SPECIAL_ROWS[i] == "clean" for i in range(8)] == [i in SPECIAL_CLEAN for i in range(8)]
    assert e["status"].tolist() == SPECIAL_STATUS[order], e["status"]
    if order == (9, 0, 0, 1):
        # the AR shortcut returns normally at a NaN model on the non-finite rows (its regression never checks them)
        for i in (1, 2, 4):
            assert np.isnan(e["coef"][i]).all() and np.isnan(e["ll"][i])
    assert np.isfinite(e["coef"][0]).all() and np.isfinite(e["coef"][7]).all()


# ---- 7. device entry and css-bobyqa boundaries --------------------------------------------------------------------
NULLS_ORDER, NULLS_N, NULLS_T = (7, 1, 2, 1), 65, 64


@functools.lru_cache(maxsize=None)
def nulls_rows():
    return _frozen(np.random.default_rng(65).standard_normal((NULLS_N, NULLS_T)).cumsum(axis=1))


@functools.lru_cache(maxsize=None)
def nulls_expect():
    return expect(nulls_rows(), *NULLS_ORDER)


def test_null_outputs_batch_converges():
    e = nulls_expect()
    assert (e["status"] == ST_OK).sum() >= NULLS_N // 2, e["status"]
    assert NULLS_N > GEN_BLOCK                               # a second workgroup, with one live lane


BOBYQA_LAST, BOBYQA_REFUSED = (6, 0, 4, 1), (6, 0, 5, 1)
BOBYQA_KMAX = 11                                             # css-bobyqa's largest compiled dimension
BOBYQA_N, BOBYQA_T = 8, 200


@functools.lru_cache(maxsize=None)
def bobyqa_rows():
    p, d, q, I = BOBYQA_LAST
    rng = np.random.default_rng(1104)
    base = [0.5, 0.2, -0.1, 0.05, 0.05, -0.02, 0.02, 0.2, 0.1, -0.05, 0.05]
    return _frozen(np.stack([O.add_time_dependent_effects(rng.standard_normal(BOBYQA_T), p, d, q, I, base)
                             for _ in range(BOBYQA_N)]))


@functools.lru_cache(maxsize=None)
def bobyqa_expect():
    return expect(bobyqa_rows(), *BOBYQA_LAST, method=1)


def test_bobyqa_sits_on_its_last_dimension():
    p, d, q, I = BOBYQA_LAST
    assert p + q + I == BOBYQA_KMAX and sum(BOBYQA_REFUSED) - BOBYQA_REFUSED[1] == BOBYQA_KMAX + 1
    e = bobyqa_expect()
    assert (e["status"] == ST_OK).sum() >= BOBYQA_N // 2, e["status"]
    assert e["n_eval"][e["status"] == ST_OK].min() > BOBYQA_KMAX + 1       # past the initial interpolation set
