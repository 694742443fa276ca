// arima_arimax.hip — ARIMAX.fitModel and ARIMAXModel.forecast (models/ARIMAX.scala) over a batch, one lane per series.
//
//   k_arimax_splice    fitModel's start point (:72-80): the ARX coefficients (AutoregressionX on the undifferenced
//                      series and the flat-differenced regressors, arima_regress.hip) with Hannan-Rissanen's last q
//                      values between the AR part and the xreg part; the ARX status wins over Hannan-Rissanen's
//   k_arimax_fit       fitWithCSSCGD (:133-161): the optimizer of k_gen_fit (one CGLane per lane, cg_lane.hpp) over all
//                      K' = 1 + p + q + nX coordinates -- its restart period `iter % n` is K' -- while the objective and
//                      the gradient read only the first ka = I + p + q of them in ARIMA's layout (:266-370). The
//                      gradient is written for all K' columns in the reference's operations: an inert column only ever
//                      receives 0 - theta * 0 and 0 * error, so it is -0.0, or NaN when the error, sigma2 or an MA
//                      coefficient is not finite or sigma2 is 0
//   k_arimax_gen_forecast  forecast(ts, xreg) (:201-256): ARIMAModel.forecast's steps with iterateARMAX (:479-541) in place
//                      of iterateARMA and the coefficients read at offset 1 whatever the intercept flag says; the last
//                      T of the T + nFuture values. The xreg term of a step is an assignment inside the loop over the
//                      predictor row (:522), so only the row's last predictor counts: the kernel reads column k - 1 of
//                      xreg and nothing else of it
//
// The fit is the correctness-first shape of DESIGN.md 4.3: per-lane arrays indexed at run time (private memory), no
// speculation. k_arimax_gen_forecast serves the orders above the compiled forecast's (p or q > 5, d > 8): it keeps the
// reference's arrays in a global workspace, one slice of series at a time, as k_gen_forecast does; at the compiled
// orders the forecast is the streaming k_arimax_forecast (arima_kernels.hip, through row_tile.hpp). tests/arimax_ref.py is the restatement both are held to bit for bit.
#include <algorithm>

#include "arima_device.hpp"
#include "arima_launch.hpp"

namespace sts {

namespace {
inline unsigned ax_grid(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }
constexpr unsigned kAxGridMax = 4096;      // single-wave workgroups, grid-stride: bounds the private memory in flight
}  // namespace

#define STS_AX_CHECK()                                                                                     \
    do {                                                                                                   \
        if (hipGetLastError() != hipSuccess) return ARIMA_E_DEVICE;                                        \
    } while (0)

// arx: N x (1 + p + nX) = (c, coefficients) of the ARX regression, hr: N x max(I + p + q, 1) of Hannan-Rissanen;
// init: N x K', arx.take(p + 1) ++ ma ++ arx.drop(p + 1) with arx(0) = 0.0 without an intercept (:75-78, :106)
__global__ void k_arimax_splice(const double *__restrict__ arx, const int32_t *__restrict__ arx_status,
                                const double *__restrict__ hr, const int32_t *__restrict__ hr_status, int64_t N, int p,
                                int q, int I, int nX, double *__restrict__ init, int32_t *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int Ka = 1 + p + nX, Kh = I + p + q, Kp = 1 + p + q + nX;
    const int st = arx_status[i] != ARIMA_ST_OK ? arx_status[i] : hr_status[i];
    status[i] = st;
    double *o = init + i * Kp;
    if (st != ARIMA_ST_OK) {
        for (int j = 0; j < Kp; ++j) o[j] = __builtin_nan("");
        return;
    }
    const double *a = arx + i * Ka;
    const double *m = hr + i * (Kh > 0 ? Kh : 1) + (Kh - q);
    o[0] = I ? a[0] : 0.0;
    for (int j = 0; j < p; ++j) o[1 + j] = a[1 + j];
    for (int j = 0; j < q; ++j) o[1 + p + j] = m[j];
    for (int j = 0; j < nX; ++j) o[1 + p + q + j] = a[1 + p + j];
}

// fitWithCSSCGD per lane (k_gen_fit's loop): the machine posts objective (F) or gradient (G) requests over K'
// coordinates, the lane serves each with one pass over its own differenced row
__global__ __launch_bounds__(64) void k_arimax_fit(const double *__restrict__ y, int64_t ld, int n, int64_t N, int p,
                                                   int q, int I, int Kp, int smear, const double *__restrict__ init,
                                                   const int32_t *__restrict__ init_status,
                                                   double *__restrict__ coef_out, double *__restrict__ ll_out,
                                                   int32_t *__restrict__ status_out, int32_t *__restrict__ n_eval_out,
                                                   int32_t *__restrict__ n_grad_out) {
    for (int64_t sid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; sid < N;
         sid += (int64_t)gridDim.x * blockDim.x) {
        const int st0 = init_status ? init_status[sid] : ARIMA_ST_OK;
        if (st0 != ARIMA_ST_OK) {
            for (int j = 0; j < Kp; ++j) coef_out[sid * Kp + j] = __builtin_nan("");
            ll_out[sid] = __builtin_nan("");
            status_out[sid] = st0;
            if (n_eval_out) n_eval_out[sid] = 0;
            if (n_grad_out) n_grad_out[sid] = 0;
            continue;
        }
        const GRow row{y + sid * ld, 0};
        GenLane L;
        L.kdim = Kp;
        double x0[kGenMaxK];
        for (int j = 0; j < kGenMaxK; ++j) x0[j] = j < Kp ? init[sid * Kp + j] : 0.0;
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
            const double css =
                req == REQ_G ? gen_grad(row, n, p, q, I, Kp, c, smear, g, dE) : gen_css(row, n, p, q, I, c);
            L.req = REQ_NONE;
            L.advance(css_to_loglik(css, n), g);
        }
        const bool ok = L.status == ARIMA_ST_OK;
        for (int j = 0; j < Kp; ++j) coef_out[sid * Kp + j] = ok ? L.point[j] : __builtin_nan("");
        ll_out[sid] = ok ? L.prev_obj : __builtin_nan("");
        status_out[sid] = L.status;
        if (n_eval_out) n_eval_out[sid] = L.n_eval;
        if (n_grad_out) n_grad_out[sid] = L.n_grad;
    }
}

// ---- ARIMAXModel.forecast (:201-256), array by array as tests/arimax_ref.py does --------------------------------
// differencesOfOrderD (UnivariateTimeSeries.scala:468-480): d passes of differencesAtLag(lag 1, start i), ping-pong
__device__ void ax_diff_d(const double *ts, int T, int d, double *out, double *tmp) {
    for (int t = 0; t < T; ++t) out[t] = ts[t];
    for (int i = 1; i <= d; ++i) {
        for (int t = 0; t < T; ++t) tmp[t] = out[t];
        for (int t = 0; t < T; ++t) out[t] = (t < i) ? tmp[t] : tmp[t] - tmp[t - 1];
    }
}

__device__ __forceinline__ void ax_update_ma(double *errs, int len, double e) {
    for (int i = 0; i < len - 1; ++i) errs[i + 1] = errs[i];
    if (len > 0) errs[0] = e;
}

// workspace per series (doubles): the arrays k_arimax_gen_forecast carves below, one spare element each
__host__ __device__ __forceinline__ int64_t ax_forecast_ws(int T, int d, int M, int nF) {
    const int64_t n = T - d, histLen = M + n, fl = nF + M, tn = T > nF ? T : nF;
    return 2 * (tn + 1) + 2 * (histLen + 1) + (fl + 1) + (int64_t)(d + 1) * T + 2 * (int64_t)(d + nF + 1) +
           ((int64_t)T + nF + 1) + (nF + 1) + (fl + 1);
}

// The xreg term of iterateARMAX's step i (`maxPQ`, :511-526): predictor row i - 1 of assemblePredictors(zeros ++ ts,
// rows of the differenced matrix, 0, L, includeOriginalXreg) exists for i - 1 < R - L (R the rows of the differenced,
// zero-prefixed matrix; transpose leaves the later rows empty) and ends with column k - 1 at time i - 1 + L
// (includeOriginalXreg) or at lag L, time i - 1; its counter is k - 1, so the weight is coefficients(p + q + k)
struct AxImpact {
    const double *xd;          // the differenced, zero-prefixed last column, R values
    int rows;                  // R - L, or 0 when a row holds no predictor at all
    int shift;                 // L with includeOriginalXreg, else 0
    double w;
    __device__ __forceinline__ double at(int i) const { return i - 1 < rows ? xd[i - 1 + shift] * w : 0.0; }
};

__global__ __launch_bounds__(64) void k_arimax_gen_forecast(const double *__restrict__ ts_all, int64_t ld_in,
                                                        const double *__restrict__ x_all, int64_t xs, int kx,
                                                        const double *__restrict__ coef_all, int Kp,
                                                        double *__restrict__ out_all, int64_t ld_out, int64_t N, int T,
                                                        int p, int d, int q, int I, int L, int orig, int nF,
                                                        double *__restrict__ ws_all, int64_t ws_stride) {
    const int64_t sid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (sid >= N) return;
    const double *ts = ts_all + sid * ld_in;
    const double *xc = x_all + sid * xs + (int64_t)(kx - 1) * nF;                       // column k - 1, nFuture values
    const double *coef = coef_all + sid * Kp;
    double *out = out_all + sid * ld_out;
    double *w = ws_all + sid * ws_stride;
    const int M = p > q ? p : q;
    const int n = T - d, histLen = M + n, fl = nF + M, Lt = T + nF, tn = T > nF ? T : nF;
    const int nd = nF > d ? nF - d : 0, R = M + nd;
    double *dts = w;                  w += tn + 1;
    double *tmp = w;                  w += tn + 1;
    double *ext = w;                  w += histLen + 1;
    double *hist = w;                 w += histLen + 1;
    double *fwd = w;                  w += fl + 1;
    double *dm = w;                   w += (int64_t)(d + 1) * T;
    double *fi = w;                   w += d + nF + 1;
    double *fo = w;                   w += d + nF + 1;
    double *res = w;                  w += (int64_t)T + nF + 1;
    double *xraw = w;                 w += nF + 1;
    double *xd = w;
    double c[kGenMaxK];
    for (int j = 0; j < kGenMaxK; ++j) c[j] = j < Kp ? coef[j] : 0.0;
    // [1] differenceXreg (:552-561) of the last column: M zeros, then the differences past the first d
    ax_diff_d(xc, nF, d, xraw, tmp);
    for (int i = 0; i < M; ++i) xd[i] = 0.0;
    for (int i = 0; i < nd; ++i) xd[M + i] = xraw[d + i];
    const bool any = L > 0 || orig;
    const AxImpact xi{xd, any ? R - L : 0, orig ? L : 0, any ? c[p + q + kx] : 0.0};
    ax_diff_d(ts, T, d, dts, tmp);                                                      // :209
    const double intercept_amt = I ? c[0] : 0.0;
    for (int i = 0; i < M; ++i) ext[i] = intercept_amt;                                 // :210
    for (int i = 0; i < n; ++i) ext[M + i] = dts[d + i];
    for (int i = 0; i < histLen; ++i) hist[i] = 0.0;
    {                                                                 // [2] iterateARMAX(ext, hist, +, gold = ext)
        double ma[kGenMaxOrder];
        for (int j = 0; j < q; ++j) ma[j] = 0.0;
        for (int i = M; i < histLen; ++i) {
            hist[i] = hist[i] + (double)I * c[0];
            for (int j = 0; j < p && i - j - 1 >= 0; ++j) hist[i] = hist[i] + ext[i - j - 1] * c[1 + j];
            hist[i] = hist[i] + xi.at(i);
            for (int j = 0; j < q; ++j) hist[i] = hist[i] + ma[j] * c[1 + p + j];
            ax_update_ma(ma, q, ext[i] - hist[i]);
        }
    }
    double maTerms[kGenMaxOrder];
    for (int i = histLen - M, j = 0; i < histLen; ++i, ++j) maTerms[j] = ext[i] - hist[i];   // [3]
    for (int i = 0; i < fl; ++i) fwd[i] = 0.0;                                          // [4]
    for (int i = 0; i < M; ++i) fwd[i] = hist[histLen - M + i];
    for (int i = M; i < fl; ++i) {                                                      // maTerms of length M
        fwd[i] = fwd[i] + (double)I * c[0];
        for (int j = 0; j < p && i - j - 1 >= 0; ++j) fwd[i] = fwd[i] + fwd[i - j - 1] * c[1 + j];
        fwd[i] = fwd[i] + xi.at(i);
        for (int j = 0; j < q; ++j) fwd[i] = fwd[i] + maTerms[j] * c[1 + p + j];
        ax_update_ma(maTerms, M, fwd[i] - fwd[i]);
    }
    for (int i = 0; i < Lt; ++i) res[i] = 0.0;                                          // [5]
    for (int i = 0; i < d && i < T; ++i) res[i] = ts[i];
    for (int i = 0; i < histLen - M; ++i) res[d + i] = hist[M + i];                     // [6]
    for (int i = 0; i < nF; ++i) res[T + i] = fwd[M + i];
    if (d != 0) {                                                                       // [7]
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
        for (int i = d; i < histLen - M; ++i) {
            double s = 0.0;
            for (int r = 0; r < d; ++r) s = s + dm[(int64_t)r * T + (i - 1)];
            res[i] = s + hist[M + i];
        }
        for (int r = 0; r < d; ++r) fi[r] = dm[(int64_t)r * T + (T - d + r)];
        for (int i = 0; i < nF; ++i) fi[d + i] = fwd[M + i];
        for (int j = 0; j < d + nF; ++j) fo[j] = fi[j];                                 // inverseDifferencesOfOrderD
        for (int lv = d; lv >= 1; --lv)
            for (int j = 0; j < d + nF; ++j) fo[j] = (j < lv) ? fo[j] : fo[j] + fo[j - 1];
        for (int i = 0; i < d + nF; ++i) res[Lt - (d + nF) + i] = fo[i];
    }
    for (int t = 0; t < T; ++t) out[t] = res[nF + t];                                   // results.drop(nFuture), :254
}

// =======================================================================================================
// launchers (arima_launch.hpp)
// =======================================================================================================
bool arimax_shape_ok(int p, int q, int Kp) { return gen_orders_ok(p, q) && Kp >= 1 && Kp <= kGenMaxK; }

int launch_arimax_splice(const double *arx, const int32_t *arx_status, const double *hr, const int32_t *hr_status,
                         int64_t N, int p, int q, int I, int nX, double *init, int32_t *status, hipStream_t s) {
    if (N == 0) return ARIMA_OK;
    if (N < 0 || !arx || !arx_status || !hr || !hr_status || !init || !status || nX < 0) return ARIMA_E_INVALID_ARG;
    hipLaunchKernelGGL(k_arimax_splice, dim3(ax_grid(N, 256)), dim3(256), 0, s, arx, arx_status, hr, hr_status, N, p, q,
                       I, nX, init, status);
    STS_AX_CHECK();
    return ARIMA_OK;
}

int launch_arimax_fit(const double *y, int64_t ld, int n, int64_t N, int p, int q, int I, int Kp, int smear,
                      const double *init, const int32_t *init_status, const FitOut &o, hipStream_t s) {
    if (!arimax_shape_ok(p, q, Kp)) return ARIMA_E_UNSUPPORTED;
    if (N == 0) return ARIMA_OK;
    if (N < 0 || n < 0 || ld < n || Kp < 1 + p + q || !y || !init || !o.coef || !o.ll || !o.status)
        return ARIMA_E_INVALID_ARG;
    const unsigned grid = std::min(ax_grid(N, 64), kAxGridMax);
    hipLaunchKernelGGL(k_arimax_fit, dim3(grid), dim3(64), 0, s, y, ld, n, N, p, q, I, Kp, smear, init, init_status,
                       o.coef, o.ll, o.status, o.n_eval, o.n_grad);
    STS_AX_CHECK();
    return ARIMA_OK;
}

int64_t arimax_forecast_ws_doubles(int T, int p, int d, int q, int n_future) {
    return ax_forecast_ws(T, d, p > q ? p : q, n_future);
}

int launch_arimax_forecast(const double *ts, int64_t ld_in, const double *x, int64_t xs, int kx, const double *coef,
                           int Kp, double *out, int64_t ld_out, int64_t N, int T, int p, int d, int q, int I, int L,
                           int orig, int n_future, double *ws, int64_t ws_stride, hipStream_t s) {
    if (!arimax_shape_ok(p, q, Kp)) return ARIMA_E_UNSUPPORTED;
    if (N == 0) return ARIMA_OK;
    const int M = p > q ? p : q;
    const int64_t R = (int64_t)M + std::max(n_future - d, 0);
    // what the kernel's indices rely on: the shapes the reference accepts (tests/arimax_ref.py forecast_check)
    if (N < 0 || M < 1 || kx < 1 || d < 0 || L < 0 || n_future < 0 || T < d || R - L < 0 || R - L > (int64_t)M + T - d ||
        Kp != 1 + p + q + kx * L + (orig ? kx : 0) || ld_in < T || ld_out < T ||
        (xs != 0 && xs < (int64_t)kx * n_future) || ws_stride < ax_forecast_ws(T, d, M, n_future) || !ts || !x ||
        !coef || !out || !ws)
        return ARIMA_E_INVALID_ARG;
    hipLaunchKernelGGL(k_arimax_gen_forecast, dim3(ax_grid(N, 64)), dim3(64), 0, s, ts, ld_in, x, xs, kx, coef, Kp, out,
                       ld_out, N, T, p, d, q, I, L, orig, n_future, ws, ws_stride);
    STS_AX_CHECK();
    return ARIMA_OK;
}

}  // namespace sts
