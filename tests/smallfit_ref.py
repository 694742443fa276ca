"""Pure-Python restatement of the EWMA and GARCH(1,1) fits (TEST INFRASTRUCTURE): the optimizer both run
(commons-math3 3.4.1 NonLinearConjugateGradientOptimizer(FLETCHER_REEVES) + LineSearch = BracketFinder +
BrentOptimizer), a literal port of oracle/arima_oracle.c's cg_optimize / line_search with the goal and the value
checker's tolerance as arguments, and each model's objective, gradient and TimeSeriesModel pair in the reference's
operation order (EWMA.scala, GARCH.scala). MINIMIZE is implemented the way commons implements it (the `isMinim ? .. : ..`
comparisons, the negated gradient), not by negating the objective, so the device code is checked against the literal
form. Every logarithm is the oracle's restated fdlibm log. Python floats are IEEE doubles and never fuse a*b+c; the
three places where Python raises instead of following IEEE (x / 0, sqrt of a negative, log) go through helpers.
"""
import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(_ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(_ROOT, "oracle"))
import oracle as O  # noqa: E402

ST_OK, ST_MAX_EVAL, ST_BRACKET_MAX_EVAL, ST_MAX_ITER, ST_BAD_INTERVAL = 0, 1, 2, 3, 7
MAX_EVAL = 10000
MAX_ITER = 10000
BRACKET_MAX = 500
NAN = float("nan")
INF = float("inf")


def jdiv(a, b):
    """a / b as Java's doubles divide (x / 0 is +-Inf or NaN, never an exception)."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return NAN
    return math.copysign(INF, a) * math.copysign(1.0, b)


def jsqrt(x):
    if x < 0.0:
        return NAN
    return math.sqrt(x)


def jlog(x):
    return O.log(x)


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


def _prec_equals(x, y):
    """Precision.equals(x, y, 1)."""
    if x != x or y != y:
        return False
    xi = int(np.float64(x).view(np.int64))
    yi = int(np.float64(y).view(np.int64))
    if (xi < 0) == (yi < 0):
        return abs(xi - yi) <= 1
    neg0 = -(1 << 63)
    if xi < yi:
        dplus, dminus = yi, xi - neg0
    else:
        dplus, dminus = xi, yi - neg0
    return False if dplus > 1 else dminus <= (1 - dplus)


def _jmax(a, b):
    if a > b:
        return a
    if a < b:
        return b
    if a != b:
        return NAN
    return a


def _value_converged(p, c, rel, abs_):
    difference = abs(p - c)
    size = _jmax(abs(p), abs(c))
    return difference <= size * rel or difference <= abs_


class _Ctx:
    def __init__(self, fobj, fgrad, minimize):
        self.fobj, self.fgrad, self.minimize = fobj, fgrad, minimize
        self.n_eval = self.n_grad = self.n_iter = 0

    def obj(self, x):
        if self.n_eval + 1 > MAX_EVAL:
            raise _Stop(ST_MAX_EVAL)
        self.n_eval += 1
        return self.fobj(x)


def _line_search(c, start, dirn):
    GOLD, EPS_MIN, grow = 1.618034, 1e-21, 100.0
    minim = c.minimize
    bcount = [0]

    def ls_f(alpha):
        return c.obj([s + alpha * d for s, d in zip(start, dirn)])

    def br_eval(alpha):
        if bcount[0] + 1 > BRACKET_MAX:
            raise _Stop(ST_BRACKET_MAX_EVAL)
        bcount[0] += 1
        return ls_f(alpha)

    def better(a, b):                       # isMinim ? a < b : a > b
        return a < b if minim else a > b

    xA, xB = 0.0, 1e-8
    fA = br_eval(xA)
    fB = br_eval(xB)
    if better(fA, fB):
        xA, xB = xB, xA
        fA, fB = fB, fA
    xC = xB + GOLD * (xB - xA)
    fC = br_eval(xC)
    while better(fC, fB):
        tmp1 = (xB - xA) * (fB - fC)
        tmp2 = (xB - xC) * (fB - fA)
        val = tmp2 - tmp1
        denom = 2 * EPS_MIN if abs(val) < EPS_MIN else val
        w = xB - ((xB - xC) * tmp2 - (xB - xA) * tmp1) / (2 * denom)
        wLim = xB + grow * (xC - xB)
        if (w - xC) * (xB - w) > 0:
            fW = br_eval(w)
            if better(fW, fC):
                xA, xB, fA, fB = xB, w, fB, fW
                break
            elif (fW > fB) if minim else (fW < fB):
                xC, fC = w, fW
                break
            w = xC + GOLD * (xC - xB)
            fW = br_eval(w)
        elif (w - wLim) * (wLim - xC) >= 0:
            w = wLim
            fW = br_eval(w)
        elif (w - wLim) * (xC - w) > 0:
            fW = br_eval(w)
            if better(fW, fC):
                xB = xC
                xC = w
                w = xC + GOLD * (xC - xB)
                fB = fC
                fC = fW
                fW = br_eval(w)
        else:
            w = xC + GOLD * (xC - xB)
            fW = br_eval(w)
        xA, fA, xB, fB, xC, fC = xB, fB, xC, fC, w, fW
    lo, mid, hi = xA, xB, xC
    if lo > hi:
        lo, hi = hi, lo
    if lo >= hi:
        raise _Stop(ST_BAD_INTERVAL)
    if mid < lo or mid > hi:
        raise _Stop(ST_BAD_INTERVAL)

    # BrentOptimizer.doOptimize
    GS = 0.5 * (3 - math.sqrt(5.0))
    relT, absT = 1e-15, 4.9e-324
    if lo < hi:
        a, b = lo, hi
    else:
        a, b = hi, lo
    x = mid
    v = x
    w = x
    d = 0.0
    e = 0.0
    fx = ls_f(x)
    if not minim:
        fx = -fx

    def best2(af, bf):                      # best(a, b, isMinim): True keeps a
        return af <= bf if minim else af >= bf

    fv = fx
    fw = fx
    have_prev = False
    prev_x = prev_f = 0.0
    cur_x, cur_f = x, (fx if minim else -fx)
    best_x, best_f = cur_x, cur_f
    while True:
        m = 0.5 * (a + b)
        tol1 = relT * abs(x) + absT
        tol2 = 2 * tol1
        stop = abs(x - m) <= tol2 - 0.5 * (b - a)
        if not stop:
            p = q = r = u = 0.0
            if abs(e) > tol1:
                r = (x - w) * (fx - fv)
                q = (x - v) * (fx - fw)
                p = (x - v) * q - (x - w) * r
                q = 2 * (q - r)
                if q > 0:
                    p = -p
                else:
                    q = -q
                r = e
                e = d
                if p > q * (a - x) and p < q * (b - x) and abs(p) < abs(0.5 * q * r):
                    d = p / q
                    u = x + d
                    if u - a < tol2 or b - u < tol2:
                        d = tol1 if x <= m else -tol1
                else:
                    e = b - x if x < m else a - x
                    d = GS * e
            else:
                e = b - x if x < m else a - x
                d = GS * e
            if abs(d) < tol1:
                u = x + tol1 if d >= 0 else x - tol1
            else:
                u = x + d
            fu = ls_f(u)
            if not minim:
                fu = -fu
            prev_x, prev_f, have_prev = cur_x, cur_f, True
            cur_x, cur_f = u, (fu if minim else -fu)
            if best2(prev_f, cur_f):
                bx2, bf2 = prev_x, prev_f
            else:
                bx2, bf2 = cur_x, cur_f
            if not best2(best_f, bf2):
                best_x, best_f = bx2, bf2
            if _value_converged(prev_f, cur_f, 1e-8, 1e-8):
                return best_x
            if fu <= fx:
                if u < x:
                    b = x
                else:
                    a = x
                v, fv, w, fw, x, fx = w, fw, x, fx, u, fu
            else:
                if u < x:
                    a = u
                else:
                    b = u
                if fu <= fw or _prec_equals(w, x):
                    v, fv, w, fw = w, fw, u, fu
                elif fu <= fv or _prec_equals(v, x) or _prec_equals(v, w):
                    v, fv = u, fu
        else:
            if have_prev:
                if best2(prev_f, cur_f):
                    bx2, bf2 = prev_x, prev_f
                else:
                    bx2, bf2 = cur_x, cur_f
                if not best2(best_f, bf2):
                    best_x, best_f = bx2, bf2
            else:
                if not best2(best_f, cur_f):
                    best_x, best_f = cur_x, cur_f
            return best_x


def cg_optimize(fobj, fgrad, init, tol, minimize):
    """NonLinearConjugateGradientOptimizer.doOptimize(FLETCHER_REEVES, SimpleValueChecker(tol, tol)) from `init`.
    fobj(x) -> float, fgrad(x) -> list. Returns dict(status, x, obj, n_eval, n_grad, n_iter); a failed fit (an
    exception in the reference) has NaN x and obj."""
    c = _Ctx(fobj, fgrad, minimize)
    k = len(init)
    point = [float(v) for v in init]

    def grad(x):
        c.n_grad += 1
        g = [float(v) for v in c.fgrad(x)]
        return [-v for v in g] if minimize else g

    try:
        r = grad(point)
        steepest = list(r)
        dirn = list(steepest)
        delta = 0.0
        for i in range(k):
            delta = delta + r[i] * dirn[i]
        have_cur = False
        cur_obj = 0.0
        while True:
            if c.n_iter + 1 > MAX_ITER:
                raise _Stop(ST_MAX_ITER)
            c.n_iter += 1
            objective = c.obj(point)
            converged = have_cur and _value_converged(cur_obj, objective, tol, tol)
            cur_obj, have_cur = objective, True
            if converged:
                return dict(status=ST_OK, x=list(point), obj=objective, n_eval=c.n_eval, n_grad=c.n_grad,
                            n_iter=c.n_iter)
            step = _line_search(c, point, dirn)
            for i in range(k):
                point[i] = point[i] + step * dirn[i]
            r = grad(point)
            delta_old = delta
            delta = 0.0
            for i in range(k):
                delta = delta + r[i] * r[i]
            beta = jdiv(delta, delta_old)
            steepest = list(r)
            if c.n_iter % k == 0 or beta < 0:
                dirn = list(steepest)
            else:
                dirn = [steepest[i] + beta * dirn[i] for i in range(k)]
    except _Stop as s:
        return dict(status=s.status, x=[NAN] * k, obj=NAN, n_eval=c.n_eval, n_grad=c.n_grad, n_iter=c.n_iter)


# ---- EWMA (EWMA.scala) ------------------------------------------------------------------------------------------
def ewma_add(ts, a):
    """EWMAModel.addTimeDependentEffects (:135-143): the recursion on dest(i - 1)."""
    n = len(ts)
    out = [0.0] * n
    if n:
        out[0] = ts[0]
    for i in range(1, n):
        out[i] = a * ts[i] + (1 - a) * out[i - 1]
    return out


def ewma_remove(ts, a):
    """EWMAModel.removeTimeDependentEffects (:125-133): reads ts(i - 1), no recursion."""
    n = len(ts)
    out = [0.0] * n
    if n:
        out[0] = ts[0]
    for i in range(1, n):
        out[i] = jdiv(ts[i] - (1 - a) * ts[i - 1], a)
    return out


def ewma_sse(ts, a):
    n = len(ts)
    smoothed = ewma_add(ts, a)
    sqr = 0.0
    for i in range(n - 1):
        error = ts[i + 1] - smoothed[i]
        sqr += error * error
    return sqr


def ewma_gradient(ts, a):
    n = len(ts)
    smoothed = ewma_add(ts, a)
    prev_smoothed = ts[0]
    prev_dsda = 0.0
    djda = 0.0
    for i in range(n - 1):
        error = ts[i + 1] - smoothed[i]
        dsda = ts[i] - prev_smoothed + (1 - a) * prev_dsda
        djda += error * dsda
        prev_dsda = dsda
        prev_smoothed = smoothed[i]
    return 2 * djda


def ewma_fit(ts):
    """EWMA.fitModel (:45-69): MINIMIZE sse from [.94], SimpleValueChecker(1e-6, 1e-6)."""
    ts = [float(v) for v in ts]
    r = cg_optimize(lambda x: ewma_sse(ts, x[0]), lambda x: [ewma_gradient(ts, x[0])], [0.94], 1e-6, True)
    return r


# ---- GARCH(1,1) (GARCH.scala) -----------------------------------------------------------------------------------
def _garch_iter(ts, omega, alpha, beta):
    prev_h = jdiv(omega, 1 - alpha - beta)
    for i in range(1, len(ts)):
        h = omega + alpha * ts[i - 1] * ts[i - 1] + beta * prev_h
        yield h, ts[i], prev_h, ts[i - 1]
        prev_h = h


def garch_loglik(ts, omega, alpha, beta):
    s = 0.0
    for h, eta, prev_h, prev_eta in _garch_iter(ts, omega, alpha, beta):
        s += -.5 * jlog(h) - jdiv(.5 * eta * eta, h)
    return s + -.5 * jlog(2 * math.pi) * (len(ts) - 1)


def garch_gradient(ts, omega, alpha, beta):
    """GARCHModel.gradient (:96-115) in the order it RETURNS: (alpha, beta, omega) halves."""
    og = ag = bg = 0.0
    od = ad = bd = 0.0
    for h, eta, prev_h, prev_eta in _garch_iter(ts, omega, alpha, beta):
        od = 1 + beta * od
        ad = prev_eta * prev_eta + beta * ad
        bd = prev_h + beta * bd
        multiplier = jdiv(eta * eta, h * h) - jdiv(1, h)
        og += multiplier * od
        ag += multiplier * ad
        bg += multiplier * bd
    return [ag * .5, bg * .5, og * .5]


def garch_remove(ts, omega, alpha, beta):
    n = len(ts)
    out = [0.0] * n
    if n == 0:
        return out
    prev_eta = ts[0]
    prev_var = jdiv(omega, 1.0 - alpha - beta)
    out[0] = jdiv(prev_eta, jsqrt(prev_var))
    for i in range(1, n):
        var = omega + alpha * prev_eta * prev_eta + beta * prev_var
        eta = ts[i]
        out[i] = jdiv(eta, jsqrt(var))
        prev_eta = eta
        prev_var = var
    return out


def garch_add(ts, omega, alpha, beta):
    n = len(ts)
    out = [0.0] * n
    if n == 0:
        return out
    prev_var = jdiv(omega, 1.0 - alpha - beta)
    prev_eta = ts[0] * jsqrt(prev_var)
    out[0] = prev_eta
    for i in range(1, n):
        var = omega + alpha * prev_eta * prev_eta + beta * prev_var
        eta = ts[i] * jsqrt(var)
        out[i] = eta
        prev_eta = eta
        prev_var = var
    return out


def garch_fit(ts):
    """GARCH.fitModel (:33-53): no GoalType, so the optimizer maximises logLikelihood from [.2, .2, .2]; the gradient's
    component 0 (alpha's) is applied to omega, 1 (beta's) to alpha, 2 (omega's) to beta -- the reference's mismatch."""
    ts = [float(v) for v in ts]
    return cg_optimize(lambda x: garch_loglik(ts, x[0], x[1], x[2]), lambda x: garch_gradient(ts, x[0], x[1], x[2]),
                       [.2, .2, .2], 1e-6, False)


def fit_batch(rows, model):
    """Fits of every row: dict(coef N x K, obj N, status, n_eval, n_grad)."""
    fit, K = (ewma_fit, 1) if model == "ewma" else (garch_fit, 3)
    N = len(rows)
    out = dict(coef=np.empty((N, K)), obj=np.empty(N), status=np.empty(N, np.int32), n_eval=np.empty(N, np.int32),
               n_grad=np.empty(N, np.int32))
    for i, row in enumerate(rows):
        r = fit(row)
        out["coef"][i] = r["x"]
        out["obj"][i] = r["obj"]
        out["status"][i], out["n_eval"][i], out["n_grad"][i] = r["status"], r["n_eval"], r["n_grad"]
    return out


# ---- fixtures (tests/golden/smallfit/*.npz) -----------------------------------------------------------------------
# EWMASuite "fitting EWMA model": the oil series of https://www.otexts.org/fpp/7/1
OIL = [446.7, 454.5, 455.7, 423.6, 456.3, 440.6, 425.3, 485.1, 506.0, 526.8, 514.3, 494.2]


def garch_rows(N, T, seed, plant=None):
    """N rows drawn from GARCH(.2, .3, .5) noise; every fourth scaled by 0.1; row 5 all zero, row 9 holds a NaN, row
    13 an Inf; `plant` (optional): a row put at index 17 (the row the search found to end in MAX_EVAL)."""
    rng = np.random.default_rng(seed)
    rows = np.empty((N, T))
    for i in range(N):
        rows[i] = garch_add(rng.standard_normal(T).tolist(), .2, .3, .5)
        if i % 4 == 3:
            rows[i] *= 0.1
    rows[5] = 0.0
    rows[9, T // 3] = NAN
    rows[13, T // 2] = INF
    if plant is not None:
        rows[17] = plant
    return rows


def planted_row_211():
    """A T = 211 row whose GARCH fit runs to MaxEval (status 1), found by searching 12000 draws of the stream below
    with the fit: draw 31 (every odd draw scaled by 0.1, like the fixture's every-fourth rows)."""
    rng = np.random.default_rng(7)
    row = None
    for _ in range(32):
        row = garch_add(rng.standard_normal(211).tolist(), .2, .3, .5)
    return np.asarray(row) * 0.1


def ewma_rows(N, T, seed):
    """Random walks, the odd rows offset by 50; row 6 constant, row 10 holds a NaN."""
    rng = np.random.default_rng(seed)
    rows = np.cumsum(rng.standard_normal((N, T)), axis=1)
    rows[1::2] += 50.0
    rows[6] = 3.25
    rows[10, T // 2] = NAN
    return rows


# name -> (model, rows): the committed fixtures; tests/golden/make_golden_smallfit.py writes them and
# tests/test_smallfit_ref.py regenerates the recorded results from the stored rows
def fixture_rows(name):
    if name == "smallfit/garch_T97":
        return "garch", garch_rows(130, 97, 1)
    if name == "smallfit/garch_T211":
        return "garch", garch_rows(130, 211, 3, plant=planted_row_211())
    if name == "smallfit/ewma_T75":
        return "ewma", ewma_rows(130, 75, 3)
    raise KeyError(name)


FIXTURES = ("smallfit/garch_T97", "smallfit/garch_T211", "smallfit/ewma_T75")
