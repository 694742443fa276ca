// gen_lane.hpp — what the runtime-order kernels share: one lane per series, per-lane arrays indexed at
// run time (private memory), correctness first.
//
//   GRow, gen_css, gen_grad, gen_model_flags   the objective, the gradient and the flags at runtime orders (also the
//                                              css-bobyqa objective above the compiled orders, arima_bobyqa_impl.hpp)
//   gen_fit_lane       fitWithCSSCGD of one series to its end: k_gen_fit (arima_generic.hip) over I + p + q coordinates,
//                      k_arimax_fit (arima_arimax.hip) over K'
//   gen_forecast_run   ARIMAModel.forecast (AX = false, k_gen_forecast) and ARIMAXModel.forecast (AX = true,
//                      k_arimax_gen_forecast), the reference's arrays in a global workspace laid out by GenFcLayout
//   gen_grid, kGenGridMax, STS_GEN_CHECK       the launchers' grid and error check
#pragma once

#include "arima_device.hpp"
#include "arima_launch.hpp"

namespace sts {

inline unsigned gen_grid(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

// fixed grids: one lane per series in single-wave workgroups, grid-stride (bounds the private memory in flight)
constexpr unsigned kGenGridMax = 4096;

#define STS_GEN_CHECK()                                                                                    \
    do {                                                                                                   \
        if (hipGetLastError() != hipSuccess) return ARIMA_E_DEVICE;                                        \
    } while (0)

// the optimizer lane: kGenMaxK padded coordinates, the first kdim real
using GenLane = CGLane<kGenMaxK, 0, 0, true, RuntimeDim>;
static_assert(sizeof(GenLane) == 8 + 8 * lane_doubles<kGenMaxK, 0, 0>() + 24, "the lane's size (cg_lane.hpp), after kdim");

// a differenced row: element i = raw[i + 1] - raw[i] (dd = 1, fused differencing) or y[i] (dd = 0)
struct GRow {
    const double *y;
    int dd;
    __device__ __forceinline__ double at(int i) const { return drow_at(y, dd, i); }
};

// ---- logLikelihoodCSSARMA's sum of squares (ARIMA.scala:430-445, iterateARMA :581-618, updateMAErrors :544-554) ----
// c has at least one entry (the intercept term multiplies c[0] even when I = 0, as css_pass does with its padded c)
__device__ double gen_css(const GRow &r, int n, int p, int q, int I, const double *c) {
    const int M = p > q ? p : q;
    double e1 = 0.0, e2 = 0.0, css = 0.0;
    const double yh0 = 0.0 + (double)I * c[0];                       // :600
    for (int t = M; t < n; ++t) {
        double yh = yh0;
        for (int j = 0; j < p; ++j) yh = yh + r.at(t - 1 - j) * c[I + j];               // :602-605
        for (int j = 0; j < q; ++j) yh = yh + (j == 0 ? e1 : e2) * c[I + p + j];        // :608-611 (ascending copy)
        const double e = r.at(t) - yh;                                                  // :613
        css = css + e * e;                                                              // :440-442
        e2 = e1;
        e1 = e;
    }
    return css;
}

// ---- gradientlogLikelihoodCSSARMA (ARIMA.scala:465-534) at runtime orders; returns the css at the same point ----
// k: the columns of dEdTheta, `coefficients.length`: I + p + q for ARIMA; ARIMAX's copy of the function
// (ARIMAX.scala:301-370) has 1 + p + q + nX, of which only the first I + p + q are ever fed (the others receive
// 0 - theta * 0 and 0 * error: -0.0, or NaN at a non-finite point).
// dE: (rows x k) scratch, rows = 2 under the Breeze smear (every lag row holds the previous row 0) and
// q + 1 under the row-shift reading. g[0..k): the gradient, already divided by -sigma2 (:532).
__device__ double gen_grad(const GRow &r, int n, int p, int q, int I, int k, const double *c, int smear, double *g,
                           double *dE) {
    const int M = p > q ? p : q;
    const int rows = smear ? (q > 0 ? 2 : 1) : q + 1;
    for (int j = 0; j < rows * k; ++j) dE[j] = 0.0;
    for (int j = 0; j < k; ++j) g[j] = 0.0;
    double e1 = 0.0, e2 = 0.0, sigma2 = 0.0, css = 0.0;
    const double nd = (double)n;
    const double yh0 = 0.0 + (double)I * c[0];
    for (int t = M; t < n; ++t) {
        for (int j = 0; j < k; ++j)                                                     // :492-499
            for (int kk = 0; kk < q; ++kk) dE[j] = dE[j] - c[I + p + kk] * dE[(smear ? 1 : kk + 1) * k + j];
        double yh = yh0;                                                                // :502
        if (k > 0) dE[0] = dE[0] - (double)I;                                           // :503
        for (int j = 0; j < p; ++j) {                                                   // :506-510
            const double v = r.at(t - 1 - j);
            yh = yh + v * c[I + j];
            dE[I + j] = dE[I + j] - v;
        }
        for (int j = 0; j < q; ++j) {                                                   // :514-518
            const double mj = (j == 0 ? e1 : e2);
            yh = yh + mj * c[I + p + j];
            dE[I + p + j] = dE[I + p + j] - mj;
        }
        const double e = r.at(t) - yh;                                                  // :520
        const double e_sq = e * e;
        sigma2 = sigma2 + e_sq / nd;                                                    // :521
        css = css + e_sq;
        e2 = e1;                                                                        // :522
        e1 = e;
        for (int j = 0; j < k; ++j) g[j] = g[j] + dE[j] * e;                            // :524
        if (smear) {                                                                    // :526, ascending element copy
            if (q > 0)
                for (int j = 0; j < k; ++j) dE[k + j] = dE[j];
        } else {                                                                        // :526, row shift
            for (int rr = q; rr >= 1; --rr)
                for (int j = 0; j < k; ++j) dE[rr * k + j] = dE[(rr - 1) * k + j];
        }
        for (int j = 0; j < k; ++j) dE[j] = 0.0;                                        // :528
    }
    for (int j = 0; j < k; ++j) g[j] = g[j] / -sigma2;                                  // :532
    return css;
}

// ---- ARIMAModel.isStationary / isInvertible (ARIMA.scala:777-815): the step-down of model_flags<P, Q, I> ----------
__device__ bool gen_roots_outside(const double *poly, int N) {
    double a[kGenMaxOrder + 1], b[kGenMaxOrder + 1];
    for (int i = 0; i <= N; ++i) {
        a[i] = poly[i];
        if (!finite(a[i])) return false;
    }
    for (int mm = N; mm >= 1; --mm) {
        const double kk = a[mm];
        if (!(fabs(kk) < 1.0)) return false;
        const double den = 1.0 - kk * kk;
        for (int i = 0; i <= N; ++i) b[i] = (i < mm) ? (a[i] - kk * a[mm - i]) / den : 0.0;
        for (int i = 0; i <= N; ++i) a[i] = b[i];
    }
    return true;
}

__device__ uint8_t gen_model_flags(const double *c, int p, int q, int I) {
    double poly[kGenMaxOrder + 1];
    bool st = true, inv = true;
    if (p > 0) {
        poly[0] = 1.0;
        for (int j = 0; j < p; ++j) poly[1 + j] = -1.0 * c[I + j];
        st = gen_roots_outside(poly, p);
    }
    if (q > 0) {
        poly[0] = 1.0;
        for (int j = 0; j < q; ++j) poly[1 + j] = c[I + p + j];
        inv = gen_roots_outside(poly, q);
    }
    return (uint8_t)((st ? ARIMA_FLAG_STATIONARY : 0) | (inv ? ARIMA_FLAG_INVERTIBLE : 0));
}

// ---- fitWithCSSCGD (ARIMA.scala:174-200) of one series to its end -------------------------------------------------
// The state machine (cg_lane.hpp) posts objective (F) or gradient (G) requests over K coordinates, of which the
// passes read the first I + p + q in ARIMA's layout; the lane serves each with one pass over its own row. x0: the
// K coordinates of the start. L is left finished (point, prev_obj, status and the counts); returns the F and G passes
// served.
struct GenPasses {
    unsigned f, g;
};

__device__ __forceinline__ GenPasses gen_fit_lane(const GRow &row, int n, int p, int q, int I, int K, int smear,
                                                  const double *__restrict__ x0_row, GenLane &L) {
    GenPasses served{0, 0};
    L.kdim = K;
    double x0[kGenMaxK];
    for (int j = 0; j < kGenMaxK; ++j) x0[j] = j < K ? x0_row[j] : 0.0;
    L.start_posted(x0);
    double g[kGenMaxK], c[kGenMaxK], dE[(kGenMaxOrder + 1) * kGenMaxK];
    for (int j = 0; j < kGenMaxK; ++j) g[j] = 0.0;
    while (!L.done()) {
        const int req = L.req;
        if (req == REQ_NONE) {                      // the machine always posts a request or finishes
            L.fail(ARIMA_ST_MAX_EVAL);
            break;
        }
        L.request_point(c);
        double css;
        if (req == REQ_G) {
            css = gen_grad(row, n, p, q, I, K, c, smear, g, dE);
            ++served.g;
        } else {
            css = gen_css(row, n, p, q, I, c);
            ++served.f;
        }
        L.req = REQ_NONE;
        L.advance(css_to_loglik(css, n), g);
    }
    return served;
}

// ---- ARIMAModel.forecast (ARIMA.scala:696-764) and ARIMAXModel.forecast (ARIMAX.scala:201-256) at any order, array
// by array as the oracle and tests/arimax_ref.py restate them ----------------------------------------------------------
// differencesOfOrderD (UnivariateTimeSeries.scala:468-480): d passes of differencesAtLag(lag 1, start i), ping-pong
__device__ void diff_d(const double *ts, int T, int d, double *out, double *tmp) {
    for (int t = 0; t < T; ++t) out[t] = ts[t];
    for (int i = 1; i <= d; ++i) {
        for (int t = 0; t < T; ++t) tmp[t] = out[t];
        for (int t = 0; t < T; ++t) out[t] = (t < i) ? tmp[t] : tmp[t] - tmp[t - 1];
    }
}

__device__ __forceinline__ void update_ma(double *errs, int len, double e) {
    for (int i = 0; i < len - 1; ++i) errs[i + 1] = errs[i];
    if (len > 0) errs[0] = e;
}

// The xreg term of iterateARMAX's step i (`maxPQ`, ARIMAX.scala:511-526): predictor row i - 1 of
// assemblePredictors(zeros ++ ts, rows of the differenced matrix, 0, L, includeOriginalXreg) exists for i - 1 < R - L
// (R the rows of the differenced, zero-prefixed matrix; transpose leaves the later rows empty) and ends with column
// k - 1 at time i - 1 + L (includeOriginalXreg) or at lag L, time i - 1; its counter is k - 1, so the weight is
// coefficients(p + q + k)
struct AxImpact {
    const double *xd;          // the differenced, zero-prefixed last column, R values
    int rows;                  // R - L, or 0 when a row holds no predictor at all
    int shift;                 // L with includeOriginalXreg, else 0
    double w;
    __device__ __forceinline__ double at(int i) const { return i - 1 < rows ? xd[i - 1 + shift] * w : 0.0; }
};

// One series' workspace: offsets of the reference's arrays (doubles, one spare element each) and their sum. ARIMAX
// differences the nFuture values of a regressor column through dts' partner tmp, and keeps three arrays of its own.
template <bool AX>
struct GenFcLayout {
    int64_t dts, tmp, ext, hist, fwd, dm, fi, fo, res, xraw, xd, size;
    __host__ __device__ GenFcLayout(int T, int d, int M, int nF) {
        const int64_t histLen = M + (T - d), fl = nF + M, tn = AX && nF > T ? nF : T;
        int64_t o = 0;
        auto take = [&o](int64_t len) {
            const int64_t at = o;
            o += len;
            return at;
        };
        dts = take(tn + 1);
        tmp = take(tn + 1);
        ext = take(histLen + 1);
        hist = take(histLen + 1);
        fwd = take(fl + 1);
        dm = take((int64_t)(d + 1) * T);
        fi = take(d + nF + 1);
        fo = take(d + nF + 1);
        res = AX ? take((int64_t)T + nF + 1) : 0;
        xraw = AX ? take(nF + 1) : 0;
        xd = AX ? take(fl + 1) : 0;
        size = o;
    }
};

// iterateARMA / iterateARMAX(src, dst, +, goldStandard = src) over [M, len) with the caller's MA terms (maLen of them,
// the first q read): dst may be src (the forward pass, whose errors are then dst[i] - dst[i])
template <bool AX>
__device__ __forceinline__ void gen_iterate(const double *src, double *dst, int M, int len, int p, int q, int I, int co,
                                            const double *c, const AxImpact &xi, double *ma, int maLen) {
    for (int i = M; i < len; ++i) {
        const double t = (double)I * c[0];
        dst[i] = dst[i] + t;
        for (int j = 0; j < p && i - j - 1 >= 0; ++j) dst[i] = dst[i] + src[i - j - 1] * c[co + j];
        if constexpr (AX) dst[i] = dst[i] + xi.at(i);         // compiled out for ARIMA: adding 0.0 would turn a -0.0 into +0.0
        for (int j = 0; j < q; ++j) dst[i] = dst[i] + ma[j] * c[co + p + j];
        update_ma(ma, maLen, src[i] - dst[i]);
    }
}

// ts: T values; coef: k coefficients, (c?, AR, MA) for ARIMA and (c, AR, MA, xreg) with c always present for ARIMAX;
// w: GenFcLayout<AX>(T, d, max(p, q), nF).size doubles. ARIMA writes the T + nF values to out. ARIMAX reads column
// kx - 1 of the regressors (xc, nF values) under xreg_max_lag L and includeOriginalXreg orig, and writes the last T of
// the T + nF values (`results.drop(nFuture)`, :254).
template <bool AX>
__device__ void gen_forecast_run(const double *__restrict__ ts, const double *__restrict__ xc, int kx,
                                 const double *__restrict__ coef, int k, double *__restrict__ out,
                                 double *__restrict__ w, int T, int p, int d, int q, int I, int L, int orig, int nF) {
    const int M = p > q ? p : q, co = AX ? 1 : I;
    const int n = T - d, histLen = M + n, fl = nF + M, Lt = T + nF;
    const GenFcLayout<AX> lay(T, d, M, nF);
    double *dts = w + lay.dts, *tmp = w + lay.tmp, *ext = w + lay.ext, *hist = w + lay.hist, *fwd = w + lay.fwd;
    double *dm = w + lay.dm, *fi = w + lay.fi, *fo = w + lay.fo;
    double *res = AX ? w + lay.res : out;
    double c[kGenMaxK];
    for (int j = 0; j < kGenMaxK; ++j) c[j] = j < k ? coef[j] : 0.0;
    AxImpact xi{nullptr, 0, 0, 0.0};
    if constexpr (AX) {      // differenceXreg (:552-561) of the last column: M zeros, then the differences past the first d
        double *xraw = w + lay.xraw, *xd = w + lay.xd;
        const int nd = nF > d ? nF - d : 0, R = M + nd;
        diff_d(xc, nF, d, xraw, tmp);
        for (int i = 0; i < M; ++i) xd[i] = 0.0;
        for (int i = 0; i < nd; ++i) xd[M + i] = xraw[d + i];
        const bool any = L > 0 || orig;
        xi = AxImpact{xd, any ? R - L : 0, orig ? L : 0, any ? c[p + q + kx] : 0.0};
    }
    diff_d(ts, T, d, dts, tmp);                                                         // ARIMA.scala:700
    const double intercept_amt = I ? c[0] : 0.0;
    for (int i = 0; i < M; ++i) ext[i] = intercept_amt;                                 // :703-707
    for (int i = 0; i < n; ++i) ext[M + i] = dts[d + i];
    for (int i = 0; i < histLen; ++i) hist[i] = 0.0;
    double ma[kGenMaxOrder];
    for (int j = 0; j < q; ++j) ma[j] = 0.0;
    gen_iterate<AX>(ext, hist, M, histLen, p, q, I, co, c, xi, ma, q);                  // :708
    for (int i = histLen - M, j = 0; i < histLen; ++i, ++j) ma[j] = ext[i] - hist[i];   // :711-713, M terms
    for (int i = 0; i < fl; ++i) fwd[i] = 0.0;
    for (int i = 0; i < M; ++i) fwd[i] = hist[histLen - M + i];                         // :717
    gen_iterate<AX>(fwd, fwd, M, fl, p, q, I, co, c, xi, ma, M);                        // :720
    for (int i = 0; i < Lt; ++i) res[i] = 0.0;
    for (int i = 0; i < d && i < T; ++i) res[i] = ts[i];                                // :724
    for (int i = 0; i < histLen - M; ++i) res[d + i] = hist[M + i];                     // :726
    for (int i = 0; i < nF; ++i) res[T + i] = fwd[M + i];                               // :728
    if (d != 0) {                                                                       // :730-762
        for (int64_t t = 0; t < (int64_t)(d + 1) * T; ++t) dm[t] = 0.0;
        for (int t = 0; t < T; ++t) dm[t] = ts[t];
        for (int i = 1; i <= d; ++i) {
            const int len = T - i;
            if (len > 0) {                  // differencesOfOrderD(row i-1 from i, 1): first kept, then differences
                const double *src = dm + (int64_t)(i - 1) * T + i;
                double *dst = dm + (int64_t)i * T + i;
                for (int t = 0; t < len; ++t) tmp[t] = src[t];
                for (int t = 0; t < len; ++t) dst[t] = (t < 1) ? tmp[t] : tmp[t] - tmp[t - 1];
            }
        }
        for (int i = d; i < histLen - M; ++i) {                                         // :745-751
            double s = 0.0;
            for (int r = 0; r < d; ++r) s = s + dm[(int64_t)r * T + (i - 1)];
            res[i] = s + hist[M + i];
        }
        for (int r = 0; r < d; ++r) fi[r] = dm[(int64_t)r * T + (T - d + r)];
        for (int i = 0; i < nF; ++i) fi[d + i] = fwd[M + i];
        for (int j = 0; j < d + nF; ++j) fo[j] = fi[j];                                 // inverseDifferencesOfOrderD
        for (int lv = d; lv >= 1; --lv)
            for (int j = 0; j < d + nF; ++j) fo[j] = (j < lv) ? fo[j] : fo[j] + fo[j - 1];
        for (int i = 0; i < d + nF; ++i) res[Lt - (d + nF) + i] = fo[i];                // :761
    }
    if constexpr (AX)
        for (int t = 0; t < T; ++t) out[t] = res[nF + t];                               // results.drop(nFuture)
}

}  // namespace sts
