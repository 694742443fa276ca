// arima_arimax.hip — ARIMAX.fitModel and ARIMAXModel.forecast (models/ARIMAX.scala) over a batch, one lane per series.
//
//   k_arimax_splice    fitModel's start point (:72-80): the ARX coefficients (AutoregressionX on the undifferenced
//                      series and the flat-differenced regressors, arima_regress.hip) with Hannan-Rissanen's last q
//                      values between the AR part and the xreg part; the ARX status wins over Hannan-Rissanen's
//   k_arimax_fit       fitWithCSSCGD (:133-161): gen_fit_lane (gen_lane.hpp), the lane loop of k_gen_fit, over all
//                      K' = 1 + p + q + nX coordinates -- its restart period `iter % n` is K' -- while the objective and
//                      the gradient read only the first ka = I + p + q of them in ARIMA's layout (:266-370). The
//                      gradient is written for all K' columns in the reference's operations: an inert column only ever
//                      receives 0 - theta * 0 and 0 * error, so it is -0.0, or NaN when the error, sigma2 or an MA
//                      coefficient is not finite or sigma2 is 0
//   k_arimax_gen_forecast  forecast(ts, xreg) (:201-256): gen_forecast_run<true> (gen_lane.hpp), ARIMAModel.forecast's
//                      steps with iterateARMAX (:479-541) in place of iterateARMA and the coefficients read at offset 1
//                      whatever the intercept flag says; the last
//                      T of the T + nFuture values. The xreg term of a step is an assignment inside the loop over the
//                      predictor row (:522), so only the row's last predictor counts: the kernel reads column k - 1 of
//                      xreg and nothing else of it
//
// The fit is the correctness-first shape of DESIGN.md 4.3: per-lane arrays indexed at run time (private memory), no
// speculation. k_arimax_gen_forecast serves the orders above the compiled forecast's (p or q > 5, d > 8): it keeps the
// reference's arrays in a global workspace, one slice of series at a time, as k_gen_forecast does; at the compiled
// orders the forecast is the streaming k_arimax_forecast (arima_kernels.hip, through row_tile.hpp). tests/arimax_ref.py
// is the restatement both are held to bit for bit.
#include <algorithm>

#include "gen_lane.hpp"

namespace sts {

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

// fitWithCSSCGD per lane over K' coordinates of its own differenced row; the reference has no flags and the runtime
// keeps no counters for this fit
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
        GenLane L;
        gen_fit_lane(GRow{y + sid * ld, 0}, n, p, q, I, Kp, smear, init + sid * Kp, L);
        const bool ok = L.status == ARIMA_ST_OK;
        for (int j = 0; j < Kp; ++j) coef_out[sid * Kp + j] = ok ? L.point[j] : __builtin_nan("");
        ll_out[sid] = ok ? L.prev_obj : __builtin_nan("");
        status_out[sid] = L.status;
        if (n_eval_out) n_eval_out[sid] = L.n_eval;
        if (n_grad_out) n_grad_out[sid] = L.n_grad;
    }
}

// ARIMAXModel.forecast (:201-256): gen_forecast_run (gen_lane.hpp) with the xreg switches, on column k - 1
__global__ __launch_bounds__(64) void k_arimax_gen_forecast(const double *__restrict__ ts_all, int64_t ld_in,
                                                        const double *__restrict__ x_all, int64_t xs, int kx,
                                                        const double *__restrict__ coef_all, int Kp,
                                                        double *__restrict__ out_all, int64_t ld_out, int64_t N, int T,
                                                        int p, int d, int q, int I, int L, int orig, int nF,
                                                        double *__restrict__ ws_all, int64_t ws_stride) {
    const int64_t sid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (sid >= N) return;
    gen_forecast_run<true>(ts_all + sid * ld_in, x_all + sid * xs + (int64_t)(kx - 1) * nF, kx, coef_all + sid * Kp, Kp,
                           out_all + sid * ld_out, ws_all + sid * ws_stride, T, p, d, q, I, L, orig, nF);
}

// =======================================================================================================
// launchers (arima_launch.hpp)
// =======================================================================================================
bool arimax_shape_ok(int p, int q, int Kp) { return gen_orders_ok(p, q) && Kp >= 1 && Kp <= kGenMaxK; }

int launch_arimax_splice(const double *arx, const int32_t *arx_status, const double *hr, const int32_t *hr_status,
                         int64_t N, int p, int q, int I, int nX, double *init, int32_t *status, hipStream_t s) {
    if (N == 0) return ARIMA_OK;
    if (N < 0 || !arx || !arx_status || !hr || !hr_status || !init || !status || nX < 0) return ARIMA_E_INVALID_ARG;
    hipLaunchKernelGGL(k_arimax_splice, dim3(gen_grid(N, 256)), dim3(256), 0, s, arx, arx_status, hr, hr_status, N, p, q,
                       I, nX, init, status);
    STS_GEN_CHECK();
    return ARIMA_OK;
}

int launch_arimax_fit(const double *y, int64_t ld, int n, int64_t N, int p, int q, int I, int Kp, int smear,
                      const double *init, const int32_t *init_status, const FitOut &o, hipStream_t s) {
    if (!arimax_shape_ok(p, q, Kp)) return ARIMA_E_UNSUPPORTED;
    if (N == 0) return ARIMA_OK;
    if (N < 0 || n < 0 || ld < n || Kp < 1 + p + q || !y || !init || !o.coef || !o.ll || !o.status)
        return ARIMA_E_INVALID_ARG;
    const unsigned grid = std::min(gen_grid(N, 64), kGenGridMax);
    hipLaunchKernelGGL(k_arimax_fit, dim3(grid), dim3(64), 0, s, y, ld, n, N, p, q, I, Kp, smear, init, init_status,
                       o.coef, o.ll, o.status, o.n_eval, o.n_grad);
    STS_GEN_CHECK();
    return ARIMA_OK;
}

int64_t arimax_forecast_ws_doubles(int T, int p, int d, int q, int n_future) {
    return GenFcLayout<true>(T, d, p > q ? p : q, n_future).size;
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
        (xs != 0 && xs < (int64_t)kx * n_future) || ws_stride < GenFcLayout<true>(T, d, M, n_future).size || !ts || !x ||
        !coef || !out || !ws)
        return ARIMA_E_INVALID_ARG;
    hipLaunchKernelGGL(k_arimax_gen_forecast, dim3(gen_grid(N, 64)), dim3(64), 0, s, ts, ld_in, x, xs, kx, coef, Kp, out,
                       ld_out, N, T, p, d, q, I, L, orig, n_future, ws, ws_stride);
    STS_GEN_CHECK();
    return ARIMA_OK;
}

}  // namespace sts
