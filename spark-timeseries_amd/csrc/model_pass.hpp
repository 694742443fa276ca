// model_pass.hpp — the one-pass recursions of the small models, one series per caller, columns consumed in time order:
// the joint objective + gradient pass of a fit and the TimeSeriesModel pair, for
//   EWMA        EWMAModel.sse / gradient / removeTimeDependentEffects / addTimeDependentEffects   (EWMA.scala:81-143)
//   GARCH(1,1)  GARCHModel.logLikelihood / gradient / iterateWithHAndEta / the pair               (GARCH.scala:82-162)
//   ARGARCH     ARGARCH.fitModel's GARCH stage on the AR(1) residuals, ARGARCHModel's pair        (GARCH.scala:63-69, 205-236)
//   AR(p)       ARModel's pair at a runtime order                                                 (Autoregression.scala:60-90)
//   and the sample recursions of GARCHModel / ARGARCHModel driven by the caller's normals         (GARCH.scala:164-185, 238-259)
// in the reference's operation order (every a * b + c is two operations: the library is built with -ffp-contract=off).
// Nothing is special-cased: a negative h gives NaN through the log, overflow gives Inf, x / 0 is IEEE's.
// Portable C++ (host and device): k_model_fit / k_model_eval / k_model_effects (arima_models.hip) and
// tests/sim/smallfit_sim.cpp and tests/sim/argarch_sim.cpp run the same code.
//
// A model has K parameters the optimizer moves and A auxiliary per-series constants it does not (Ewma, Garch: A = 0;
// ArGarch: A = 2, the AR stage's (c, phi)). Pass::begin(x, aux) takes both; a parameter block of the pair (Fx::begin)
// is the A constants followed by the K parameters, NP = A + K doubles.
//
// GARCH's gradient keeps the reference's order: GARCHModel.gradient RETURNS (alpha, beta, omega) halves (:114) while
// GARCH.fitModel's parameters are (omega, alpha, beta) (:40-41), so the optimizer applies alpha's derivative to omega,
// beta's to alpha and omega's to beta. That mismatch is the reference's; a drop-in returns what spark-ts returns.
#pragma once

#include <stdint.h>

#include "cg_small.hpp"

namespace sts {
namespace small {

// fdlibm __ieee754_log (java.lang.StrictMath.log; arima_device.hpp dlog / oracle orc_log), host and device
STS_SM_HD double sm_log(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10,
                 two54 = 1.80143985094819840000e+16, Lg1 = 6.666666666666735130e-01,
                 Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                 Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01,
                 Lg6 = 1.531383769920937332e-01, Lg7 = 1.479819860511658591e-01;
    const double zero = 0.0;
    int64_t bits = __builtin_bit_cast(int64_t, x);
    int32_t hx = (int32_t)(bits >> 32);
    const uint32_t lx = (uint32_t)bits;
    int32_t k = 0;
    if (hx < 0x00100000) {
        if (((hx & 0x7fffffff) | lx) == 0) return -two54 / zero;
        if (hx < 0) return (x - x) / zero;
        k -= 54;
        x *= two54;
        hx = (int32_t)(__builtin_bit_cast(int64_t, x) >> 32);
    }
    if (hx >= 0x7ff00000) return x + x;
    k += (hx >> 20) - 1023;
    hx &= 0x000fffff;
    int32_t i = (hx + 0x95f64) & 0x100000;
    {
        uint64_t u = __builtin_bit_cast(uint64_t, x);
        u = ((uint64_t)(uint32_t)(hx | (i ^ 0x3ff00000)) << 32) | (u & 0xffffffffull);
        x = __builtin_bit_cast(double, u);
    }
    k += (i >> 20);
    const double f = x - 1.0;
    double dk;
    if ((0x000fffff & (2 + hx)) < 3) {
        if (f == 0.0) {
            if (k == 0) return 0.0;
            dk = (double)k;
            return dk * ln2_hi + dk * ln2_lo;
        }
        const double R = f * f * (0.5 - 0.33333333333333333 * f);
        if (k == 0) return f - R;
        dk = (double)k;
        return dk * ln2_hi - ((R - dk * ln2_lo) - f);
    }
    const double s = f / (2.0 + f);
    dk = (double)k;
    const double z = s * s;
    i = hx - 0x6147a;
    const double w = z * z;
    const int32_t j = 0x6b851 - hx;
    const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
    const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
    i |= j;
    const double R = t2 + t1;
    if (i > 0) {
        const double hfsq = 0.5 * f * f;
        if (k == 0) return f - (hfsq - s * (hfsq + R));
        return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
    }
    if (k == 0) return f - s * (f - R);
    return dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}

// ---------------------------------------------------------------------------------------------------------------
// EWMA: one parameter, `smoothing`; MINIMIZE sse from [.94]
// ---------------------------------------------------------------------------------------------------------------
struct Ewma {
    static constexpr int K = 1, A = 0, NP = K + A;
    static constexpr bool kMinimize = true;                  // val goal = GoalType.MINIMIZE (EWMA.scala:64)
    STS_SM_HD static void initial_guess(double *x) { x[0] = .94; }

    // sse (:81-96) and gradient (:102-123) in one pass. Both build `smoothed` first (addTimeDependentEffects) and then
    // loop over i < n - 1 reading ts(i + 1), smoothed(i), ts(i) and smoothed(i - 1): at column t = i + 1 those are the
    // column, and three values carried from columns t - 1 and t - 2.
    struct Pass {
        double a, om;            // smoothing, 1 - smoothing
        double s, xp, ps;        // smoothed(t - 1), ts(t - 1), prevSmoothed
        double pd, dj, sq;       // prevDSda, dJda, sqrErrors
        STS_SM_HD void begin(const double *x, const double * = nullptr) {
            a = x[0];
            om = 1 - a;
            s = xp = ps = 0.0;
            pd = dj = sq = 0.0;
        }
        STS_SM_HD void step(int t, double v) {
            if (t == 0) {
                s = v;               // arr(0) = ts(0)
                ps = v;              // var prevSmoothed = ts(0)
            } else {
                const double error = v - s;                   // ts(i + 1) - smoothed(i)
                sq = sq + error * error;
                const double ds = xp - ps + om * pd;          // ts(i) - prevSmoothed + (1 - smoothing) * prevDSda
                dj = dj + error * ds;
                pd = ds;
                ps = s;
                s = a * v + om * s;                           // smoothing * ts(i) + (1 - smoothing) * dest(i - 1)
            }
            xp = v;
        }
        STS_SM_HD void end(int T, double *f, double *g) const {
            *f = sq;
            g[0] = 2 * dj;
        }
    };

    // removeTimeDependentEffects (:125-133; reads ts(i - 1)) / addTimeDependentEffects (:135-143; recursion on dest)
    template <bool ADD>
    struct Fx {
        double a, om, prev;
        STS_SM_HD void begin(const double *x) { a = x[0]; om = 1 - a; prev = 0.0; }
        STS_SM_HD double step(int t, double v) {
            double o;
            if (t == 0) o = v;
            else o = ADD ? a * v + om * prev : (v - om * prev) / a;
            prev = ADD ? o : v;
            return o;
        }
    };
};

// ---------------------------------------------------------------------------------------------------------------
// GARCH(1,1): parameters (omega, alpha, beta); no GoalType, so commons maximises logLikelihood from [.2, .2, .2]
// ---------------------------------------------------------------------------------------------------------------
struct Garch {
    static constexpr int K = 3, A = 0, NP = K + A;
    static constexpr bool kMinimize = false;
    STS_SM_HD static void initial_guess(double *x) { x[0] = .2; x[1] = .2; x[2] = .2; }

    // logLikelihood (:82-88) and gradient (:96-115) over iterateWithHAndEta (:117-129) in one pass
    struct Pass {
        double omega, alpha, beta;
        double ph, xp;                   // prevH, ts(i - 1)
        double sum, og, ag, bg;          // the log-likelihood sum; omega / alpha / betaGradient
        double od, ad, bd;               // omega / alpha / betaDhdtheta
        STS_SM_HD void begin(const double *x, const double * = nullptr) {
            omega = x[0]; alpha = x[1]; beta = x[2];
            ph = omega / (1 - alpha - beta);
            xp = 0.0;
            sum = og = ag = bg = 0.0;
            od = ad = bd = 0.0;
        }
        STS_SM_HD void step(int t, double v) {
            if (t > 0) {
                const double h = omega + alpha * xp * xp + beta * ph;
                sum = sum + (-.5 * sm_log(h) - .5 * v * v / h);
                od = 1 + beta * od;
                ad = xp * xp + beta * ad;
                bd = ph + beta * bd;
                const double mult = (v * v / (h * h)) - (1 / h);
                og = og + mult * od;
                ag = ag + mult * ad;
                bg = bg + mult * bd;
                ph = h;
            }
            xp = v;
        }
        STS_SM_HD void end(int T, double *f, double *g) const {
            *f = sum + -.5 * sm_log(2 * 3.141592653589793) * (double)(T - 1);
            g[0] = ag * .5;              // Array(alphaGradient * .5, betaGradient * .5, omegaGradient * .5)
            g[1] = bg * .5;
            g[2] = og * .5;
        }
    };

    // removeTimeDependentEffects (:131-145) / addTimeDependentEffects (:147-162)
    template <bool ADD>
    struct Fx {
        double omega, alpha, beta, pe, pv;       // prevEta, prevVariance
        STS_SM_HD void begin(const double *x) {
            omega = x[0]; alpha = x[1]; beta = x[2];
            pv = omega / (1.0 - alpha - beta);
            pe = 0.0;
        }
        STS_SM_HD double step(int t, double v) {
            if (t > 0) pv = omega + alpha * pe * pe + beta * pv;
            const double sd = __builtin_sqrt(pv);
            const double o = ADD ? v * sd : v / sd;
            pe = ADD ? o : v;
            return o;
        }
    };
};

// ---------------------------------------------------------------------------------------------------------------
// ARGARCH: AR(1) with an intercept, GARCH(1,1) errors. The optimizer's parameters are Garch's; (c, phi) come from the
// AR stage (Autoregression.fitModel) and stay fixed, so the fit is Garch's on the residuals
//   r(0) = ts(0) - c,  r(i) = (ts(i) - c) - ts(i - 1) * phi      (ARModel.removeTimeDependentEffects, p = 1)
// formed per column from the raw row: two roundings, in that order. The residual row is never stored.
// ---------------------------------------------------------------------------------------------------------------
struct ArGarch {
    static constexpr int K = 3, A = 2, NP = K + A;
    static constexpr bool kMinimize = false;
    STS_SM_HD static void initial_guess(double *x) { Garch::initial_guess(x); }

    struct Pass {
        Garch::Pass g;
        double c, phi, pv;               // pv: ts(t - 1), the raw value
        STS_SM_HD void begin(const double *x, const double *aux) {
            g.begin(x);
            c = aux[0]; phi = aux[1];
            pv = 0.0;
        }
        STS_SM_HD void step(int t, double v) {
            double r = v - c;
            if (t > 0) r = r - pv * phi;
            pv = v;
            g.step(t, r);
        }
        STS_SM_HD void end(int T, double *f, double *gr) const { g.end(T, f, gr); }
    };

    // ARGARCHModel.removeTimeDependentEffects (:205-219) / addTimeDependentEffects (:221-236; recursion on dest(i - 1));
    // x = (c, phi, omega, alpha, beta)
    template <bool ADD>
    struct Fx {
        double c, phi, omega, alpha, beta, pe, pv, pr;       // prevEta, prevVariance; pr: ts(i - 1) / dest(i - 1)
        STS_SM_HD void begin(const double *x) {
            c = x[0]; phi = x[1]; omega = x[2]; alpha = x[3]; beta = x[4];
            pv = omega / (1.0 - alpha - beta);
            pe = pr = 0.0;
        }
        STS_SM_HD double step(int t, double v) {
            if (t > 0) pv = omega + alpha * pe * pe + beta * pv;
            const double sd = __builtin_sqrt(pv);
            double o;
            if (ADD) {
                pe = v * sd;
                o = t > 0 ? c + phi * pr + pe : c + pe;
                pr = o;
            } else {
                pe = t > 0 ? v - c - phi * pr : v - c;
                o = pe / sd;
                pr = v;
            }
            return o;
        }
    };
};

// ---------------------------------------------------------------------------------------------------------------
// ARModel's pair at order p <= kArMaxP (Autoregression.scala:60-90): dest(i) = ts(i) - c (remove) or c + ts(i) (add),
// then one lag at a time, j ascending, only the lags that exist (i - j - 1 >= 0). `coef` = (c, phi_1 .. phi_p).
// hist (the caller's, p doubles: a runtime-indexed array belongs in LDS on the device, not in registers) is a ring of
// the last p raw values (remove) or outputs (add): value t lives at hist[t % p].
// ---------------------------------------------------------------------------------------------------------------
constexpr int kArMaxP = 20;
template <bool ADD>
struct ArFx {
    int p;
    const double *coef;
    double *hist;
    STS_SM_HD void begin(const double *coef_, int p_, double *hist_) { coef = coef_; p = p_; hist = hist_; }
    STS_SM_HD double step(int t, double v) {
        double o = ADD ? coef[0] + v : v - coef[0];
        const int lags = t < p ? t : p;
        int k = t % p;                               // slot of value t; value t - j - 1 is j + 1 slots before it
        const int slot = k;
        for (int j = 0; j < lags; ++j) {
            k = k == 0 ? p - 1 : k - 1;
            o = ADD ? o + hist[k] * coef[1 + j] : o - hist[k] * coef[1 + j];
        }
        hist[slot] = ADD ? o : v;
        return o;
    }
};

// ---------------------------------------------------------------------------------------------------------------
// GARCHModel.sample / ARGARCHModel.sample (GARCH.scala:164-185, 238-259) with the gaussians pre-drawn: z(t) is the
// t-th nextGaussian(). ts(0) is never assigned (0.0), z(0) only feeds variances(1); the variance recursion here is
// omega + beta * v + alpha * eta * eta, not the pair's order. AR: x = (c, phi, omega, alpha, beta), else (omega, alpha, beta)
// ---------------------------------------------------------------------------------------------------------------
template <bool AR>
struct GarchSample {
    static constexpr int NP = AR ? 5 : 3;
    double c, phi, omega, alpha, beta, var, eta, prev;
    STS_SM_HD void begin(const double *x) {
        c = AR ? x[0] : 0.0; phi = AR ? x[1] : 0.0;
        omega = x[NP - 3]; alpha = x[NP - 2]; beta = x[NP - 1];
        var = omega / (1 - alpha - beta);
        eta = prev = 0.0;
    }
    STS_SM_HD double step(int t, double z) {
        if (t > 0) var = omega + beta * var + alpha * eta * eta;
        eta = __builtin_sqrt(var) * z;
        if (t == 0) return 0.0;
        prev = AR ? c + phi * prev + eta : eta;
        return prev;
    }
};

}  // namespace small
}  // namespace sts
