"""Pure-Python restatement of ARGARCH.fitModel, the ARModel and ARGARCHModel TimeSeriesModel pairs and the three `sample`
recursions (TEST INFRASTRUCTURE), in the reference's operation order (GARCH.scala:56-70, 164-185, 198-260;
Autoregression.scala:56-96). The AR stage is the oracle's Autoregression.fitModel (oracle.ar_fit), the GARCH stage
tests/smallfit_ref.py's garch_fit; Python floats are IEEE doubles and never fuse a * b + c, and the operations where
Python raises instead of following IEEE go through smallfit_ref's jdiv / jsqrt / jlog.

`sample` takes the gaussians pre-drawn: z[t] is the t-th rand.nextGaussian() of the reference's loop.
"""
import numpy as np

import oracle as O
import smallfit_ref as S
from smallfit_ref import jdiv, jlog, jsqrt  # noqa: F401  (jlog: re-exported for callers that restate logLikelihood)

NAN = float("nan")
ST_OK, ST_MAX_EVAL = S.ST_OK, S.ST_MAX_EVAL
ST_SINGULAR, ST_NOT_ENOUGH_DATA, ST_NO_DATA = 4, 5, 6


# ---- ARModel (Autoregression.scala:60-96) -----------------------------------------------------------------------------
def ar_remove(ts, c, coefficients):
    """ARModel.removeTimeDependentEffects: dest(i) = ts(i) - c, then dest(i) -= ts(i - j - 1) * coefficients(j) for the
    lags that exist, j ascending."""
    n = len(ts)
    out = [0.0] * n
    for i in range(n):
        v = ts[i] - c
        j = 0
        while j < len(coefficients) and i - j - 1 >= 0:
            v = v - ts[i - j - 1] * coefficients[j]
            j += 1
        out[i] = v
    return out


def ar_add(ts, c, coefficients):
    """ARModel.addTimeDependentEffects: dest(i) = c + ts(i), then dest(i) += dest(i - j - 1) * coefficients(j)."""
    n = len(ts)
    out = [0.0] * n
    for i in range(n):
        v = c + ts[i]
        j = 0
        while j < len(coefficients) and i - j - 1 >= 0:
            v = v + out[i - j - 1] * coefficients[j]
            j += 1
        out[i] = v
    return out


def ar_sample(z, c, coefficients):
    """ARModel.sample: addTimeDependentEffects(vec, vec) in place -- step i reads ts(i) before writing dest(i) and only
    written entries after, so the out-of-place form yields the same values."""
    return ar_add(z, c, coefficients)


# ---- ARGARCHModel (GARCH.scala:198-260) -------------------------------------------------------------------------------
def argarch_remove(ts, c, phi, omega, alpha, beta):
    n = len(ts)
    out = [0.0] * n
    if n == 0:
        return out
    prev_eta = ts[0] - c
    prev_var = jdiv(omega, 1.0 - alpha - beta)
    out[0] = jdiv(prev_eta, jsqrt(prev_var))
    for i in range(1, n):
        var = omega + alpha * prev_eta * prev_eta + beta * prev_var
        eta = ts[i] - c - phi * ts[i - 1]
        out[i] = jdiv(eta, jsqrt(var))
        prev_eta = eta
        prev_var = var
    return out


def argarch_add(ts, c, phi, omega, alpha, beta):
    n = len(ts)
    out = [0.0] * n
    if n == 0:
        return out
    prev_var = jdiv(omega, 1.0 - alpha - beta)
    prev_eta = ts[0] * jsqrt(prev_var)
    out[0] = c + prev_eta
    for i in range(1, n):
        var = omega + alpha * prev_eta * prev_eta + beta * prev_var
        eta = ts[i] * jsqrt(var)
        out[i] = c + phi * out[i - 1] + eta
        prev_eta = eta
        prev_var = var
    return out


def _sample(z, c, phi, omega, alpha, beta, ar):
    n = len(z)
    ts = [0.0] * n
    if n == 0:
        return ts
    var = jdiv(omega, 1 - alpha - beta)
    eta = jsqrt(var) * z[0]
    for i in range(1, n):
        var = omega + beta * var + alpha * eta * eta
        eta = jsqrt(var) * z[i]
        ts[i] = c + phi * ts[i - 1] + eta if ar else eta
    return ts


def garch_sample(z, omega, alpha, beta):
    """GARCHModel.sample (:164-185): ts(0) stays 0.0, the first draw only feeds variances(1)."""
    return _sample(z, 0.0, 0.0, omega, alpha, beta, False)


def argarch_sample(z, c, phi, omega, alpha, beta):
    """ARGARCHModel.sample (:238-259): ts(i) = c + phi * ts(i - 1) + eta."""
    return _sample(z, c, phi, omega, alpha, beta, True)


# ---- ARGARCH.fitModel (GARCH.scala:63-69) -----------------------------------------------------------------------------
def argarch_fit(ts):
    """dict(status, x = [c, phi, omega, alpha, beta], obj = logLikelihood of the residuals, n_eval, n_grad, ar_status).
    A series either stage throws on has no model: NaN x and obj; when the AR stage threw, the counters are 0."""
    ts = [float(v) for v in ts]
    st, c, coef = O.ar_fit(ts, 1)
    if st != ST_OK:
        return dict(status=int(st), x=[NAN] * 5, obj=NAN, n_eval=0, n_grad=0, ar_status=int(st))
    phi = float(coef[0])
    g = S.garch_fit(ar_remove(ts, c, [phi]))
    x = [c, phi] + list(g["x"]) if g["status"] == ST_OK else [NAN] * 5
    return dict(status=g["status"], x=x, obj=g["obj"], n_eval=g["n_eval"], n_grad=g["n_grad"], ar_status=ST_OK)


def fit_batch(rows):
    """ARGARCH fits of every row: dict(coef N x 5, obj N, status, n_eval, n_grad, ar_status)."""
    N = len(rows)
    out = dict(coef=np.empty((N, 5)), obj=np.empty(N), status=np.empty(N, np.int32), n_eval=np.empty(N, np.int32),
               n_grad=np.empty(N, np.int32), ar_status=np.empty(N, np.int32))
    for i, row in enumerate(rows):
        r = argarch_fit(row)
        out["coef"][i] = r["x"]
        out["obj"][i] = r["obj"]
        for k in ("status", "n_eval", "n_grad", "ar_status"):
            out[k][i] = r[k]
    return out


# ---- fixtures (tests/golden/argarch/*.npz) ----------------------------------------------------------------------------
PHIS = (-0.6, 0.0, 0.4, 0.9)


def argarch_rows(N, T, seed):
    """N rows from ARGARCHModel(c, phi, .2, .3, .5).addTimeDependentEffects on default_rng(seed) normals, c = 0.5 *
    (i % 3), phi = PHIS[i % 4]; every fourth scaled by 0.1; row 5 all zero, row 6 constant, row 9 holds a NaN, row 13
    an Inf."""
    rng = np.random.default_rng(seed)
    rows = np.empty((N, T))
    for i in range(N):
        rows[i] = argarch_add(rng.standard_normal(T).tolist(), 0.5 * (i % 3), PHIS[i % 4], .2, .3, .5)
        if i % 4 == 3:
            rows[i] *= 0.1
    rows[5] = 0.0
    rows[6] = 3.25
    rows[9, T // 3] = NAN
    rows[13, T // 2] = float("inf")
    return rows


# name -> rows: the committed fixtures; tests/golden/make_golden_argarch.py writes them and tests/test_argarch_ref.py
# regenerates the recorded results from the stored rows
_FIXTURE_SHAPES = {"argarch/argarch_T97": (130, 97, 1), "argarch/argarch_T211": (70, 211, 3)}
FIXTURES = tuple(_FIXTURE_SHAPES)


def fixture_rows(name):
    return argarch_rows(*_FIXTURE_SHAPES[name])


def suite_pattern(n):
    """GARCHSuite "fit model 2": the period-8 pattern repeated to n values."""
    base = (0.1, -0.2, -0.1, 0.1, 0.0, -0.01, 0.0, -0.1)
    return [base[i % 8] for i in range(n)]


# ---- shared inputs and expected outputs of the pair / sample tests (CPU sim and GPU) ----------------------------------
AR_ORDERS = (1, 2, 5, 20)
_PAIRS = {}


def pair_params(N):
    """(N x 5 ARGARCH parameters, {p: N x (1 + p) AR coefficients}) with special values in the first rows."""
    rng = np.random.default_rng(77)
    g = np.stack([rng.uniform(-1, 1, N), rng.uniform(-.9, .9, N), rng.uniform(.05, .5, N), rng.uniform(.05, .4, N),
                  rng.uniform(.05, .5, N)], axis=1)
    g[0] = (40.0, .4, .2, .3, .4)                            # GARCHSuite "standardize and filter"
    g[1, 1] = float("inf")                                   # phi = Inf: step 0 must not touch it
    g[2, 3:] = (.5, .5)                                      # alpha + beta = 1: prevVariance = omega / 0
    g[3, 2] = NAN
    g[4, 3] = -.2
    g[5, 0] = NAN
    ar = {}
    for p in AR_ORDERS:
        a = np.concatenate([rng.uniform(-1, 1, (N, 1)), rng.uniform(-1, 1, (N, p)) / p], axis=1)
        a[1, 1] = float("inf")
        a[3, p] = NAN
        a[4, 1:] = 1.0                                       # grows like p ** t: overflows to Inf at the longer T
        ar[p] = a
    return g, ar


def pair_reference(T, N=130):
    """The restatement's pairs and samples over N rows of length T (computed once per T and left unchanged): rows (also
    the normals of the samples), g, ar, and the expected N x T outputs by name."""
    if (T, N) not in _PAIRS:
        rng = np.random.default_rng(2000 + T)
        rows = rng.standard_normal((N, T))
        rows[8] *= 1e160                                     # overflows to Inf in the squares
        if T > 2:
            rows[9, T // 2] = NAN
        g, ar = pair_params(N)
        rl, gl = rows.tolist(), g.tolist()                   # Python floats: IEEE results without numpy's warnings
        ref = dict(rows=rows, g=g, ar=ar,
                   argarch_remove=np.array([argarch_remove(r, *c) for r, c in zip(rl, gl)]),
                   argarch_add=np.array([argarch_add(r, *c) for r, c in zip(rl, gl)]),
                   argarch_sample=np.array([argarch_sample(r, *c) for r, c in zip(rl, gl)]),
                   garch_sample=np.array([garch_sample(r, *c[2:]) for r, c in zip(rl, gl)]))
        for p in AR_ORDERS:
            al = ar[p].tolist()
            ref[f"ar_remove_{p}"] = np.array([ar_remove(r, a[0], a[1:]) for r, a in zip(rl, al)])
            ref[f"ar_add_{p}"] = np.array([ar_add(r, a[0], a[1:]) for r, a in zip(rl, al)])
        _PAIRS[(T, N)] = ref
    return _PAIRS[(T, N)]
