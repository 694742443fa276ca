// arima_chisq.hpp — the chi-squared upper tail the reference's tests report as their p-value (host and device):
//   1 - new ChiSquaredDistribution(L).cumulativeProbability(stat)      (TimeSeriesStatisticalTests.scala:298-307)
// restated from commons-math3 3.4.1: GammaDistribution.cumulativeProbability (0 for x <= 0, else
// Gamma.regularizedGammaP(L / 2, x / 2) at epsilon 1e-15, Integer.MAX_VALUE iterations), regularizedGammaP (the series
// for x < a + 1, else 1 - regularizedGammaQ), regularizedGammaQ (the continued fraction a_n = 2n + 1 - a + x,
// b_n = n (a - n) in ContinuedFraction.evaluate's modified Lentz form) and Gamma.logGamma.
//
// NOT bit-exact, by construction: the JVM evaluates exp and log with FastMath, whose last bits no libm reproduces, so
// the p-value is the one output of the diagnostics held to a tolerance and not to bits. Two more
// departures, both inside that tolerance:
//   - logGamma(a) for a <= 8 is, in the library, the NSWC polynomial logGamma1p; chi-squared only ever asks for
//     a = L / 2, where Gamma has a closed form (a factorial, or sqrt(pi) times a product of half-integers, exact in
//     fp64 up to a = 8), so that is what is evaluated here. Above 8 it is the library's Lanczos sum.
//   - where the library throws (a statistic of +Inf makes the continued fraction NaN), a batch cannot: the p-value of
//     that row is NaN. NaN in gives NaN out, as in the library.
// The tolerance is 2.31e-14 up to L = 40 and 2.21e-13 above (measured up to L = 255).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define STS_CHISQ_HD __host__ __device__
#else
#define STS_CHISQ_HD
#endif

namespace sts {

constexpr double kChisqEps = 1e-15;                       // GammaDistribution's default absolute accuracy
constexpr double kHalfLogPi = 0.5723649429247001;         // log(sqrt(pi))
constexpr double kHalfLog2Pi = 0.9189385332046727;        // Gamma.HALF_LOG_2_PI
constexpr double kLanczosG = 607.0 / 128.0;               // Gamma.LANCZOS_G

// Gamma.lanczos: summed from the last coefficient down, the constant term last
STS_CHISQ_HD inline double chisq_lanczos(double x) {
    const double c[15] = {0.99999999999999709182,  57.156235665862923517,   -59.597960355475491248,
                          14.136097974741747174,   -0.49191381609762019978, .33994649984811888699e-4,
                          .46523628927048575665e-4, -.98374475304879564677e-4, .15808870322491248884e-3,
                          -.21026444172410488319e-3, .21743961811521264320e-3, -.16431810653676389022e-3,
                          .84418223983852743293e-4, -.26190838401581408670e-4, .36899182659531622704e-5};
    double sum = 0.0;
    for (int i = 14; i > 0; --i) sum += c[i] / (x + i);
    return sum + c[0];
}

// logGamma(L / 2), L >= 1
STS_CHISQ_HD inline double chisq_log_gamma_half(int32_t L) {
    const double a = 0.5 * (double)L;
    if (a <= 8.0) {
        double prod = 1.0;
        if (L % 2 == 0) {
            for (int i = 2; i < L / 2; ++i) prod *= (double)i;                  // Gamma(n) = (n - 1)!
            return log(prod);
        }
        for (int j = 1; j <= (L - 1) / 2; ++j) prod *= (double)j - 0.5;         // Gamma(n + 1/2) / sqrt(pi)
        return kHalfLogPi + log(prod);
    }
    const double sum = chisq_lanczos(a);
    const double tmp = a + kLanczosG + .5;
    return ((a + .5) * log(tmp)) - tmp + kHalfLog2Pi + log(sum / a);
}

// Gamma.regularizedGammaP's series, x < a + 1
STS_CHISQ_HD inline double chisq_gamma_p_series(double a, double x, double lg) {
    double n = 0.0, an = 1.0 / a, sum = an;
    while (fabs(an / sum) > kChisqEps && n < 2147483647.0 && sum < INFINITY) {
        n += 1.0;
        an *= x / (a + n);
        sum += an;
    }
    if (isinf(sum)) return 1.0;
    return exp(-x + (a * log(x)) - lg) * sum;
}

// Gamma.regularizedGammaQ's continued fraction, x >= a + 1 (ContinuedFraction.evaluate, small = 1e-50)
STS_CHISQ_HD inline double chisq_gamma_q_cf(double a, double x, double lg) {
    const double small = 1e-50;
    double hPrev = 1.0 - a + x;
    if (fabs(hPrev) <= small) hPrev = small;
    double dPrev = 0.0, cPrev = hPrev, hN = hPrev;
    for (int n = 1; n < 2147483647; ++n) {
        const double an = ((2.0 * n) + 1.0) - a + x;
        const double bn = n * (a - n);
        double dN = an + bn * dPrev;
        if (fabs(dN) <= small) dN = small;
        double cN = an + bn / cPrev;
        if (fabs(cN) <= small) cN = small;
        dN = 1 / dN;
        const double deltaN = cN * dN;
        hN = hPrev * deltaN;
        if (isinf(hN) || isnan(hN)) return NAN;                                 // the library throws
        if (fabs(deltaN - 1.0) < kChisqEps) break;
        dPrev = dN;
        cPrev = cN;
        hPrev = hN;
    }
    return exp(-x + (a * log(x)) - lg) * (1.0 / hN);
}

// 1 - ChiSquaredDistribution(L).cumulativeProbability(stat), L >= 1
STS_CHISQ_HD inline double chisq_upper_tail(int32_t L, double stat) {
    if (isnan(stat)) return NAN;
    if (stat <= 0.0) return 1.0 - 0.0;                                          // cumulativeProbability is 0
    const double a = (double)L / 2.0, x = stat / 2.0;
    const double lg = chisq_log_gamma_half(L);
    double cdf;
    if (x >= a + 1.0)
        cdf = 1.0 - chisq_gamma_q_cf(a, x, lg);
    else
        cdf = chisq_gamma_p_series(a, x, lg);
    return 1.0 - cdf;
}

}  // namespace sts
