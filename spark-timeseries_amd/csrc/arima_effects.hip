// arima_effects.hip — the TimeSeriesModel pair of ARIMAModel (TimeSeriesModel.scala:23-45) over a batch:
//   remove  ARIMAModel.removeTimeDependentEffects (ARIMA.scala:629-644): the residuals of a series under a model
//   add     ARIMAModel.addTimeDependentEffects    (ARIMA.scala:655-667): a model driven by the caller's innovations
// One lane per series, one streaming pass: every element is read once and written once, and everything the reference
// materialises as an array is carried in registers:
//   Dp[r]   = D(r, t-1), the differencing column (differencesOfOrderD, UnivariateTimeSeries.scala:468-480; remove)
//   Ip[l]   = the running sum of integration pass l+1 at t-1 (inverseDifferencesOfOrderD, :489-495; add) -- the d
//             in-place passes of the reference become d cascaded running sums, the same additions in the same order
//   hist[j] = the AR operand at t-1-j: the differenced series (remove) or the values already produced, before
//             integration (add); the intercept amount before t = 0 (ARIMA.scala:633-636, :659-661)
//   ma[j]   = the error terms (updateMAErrors, ARIMA.scala:544-554: the ascending copy, a smear)
// Same operations in the same order as oracle/arima_oracle.c (orc_remove_time_dependent_effects,
// orc_add_time_dependent_effects), so the result is bit-identical.
//
// Memory path: row_tile.hpp (RowTile<32>::map). Output t is final at step t; the output may be the input.
// Templated on max(p, q) and the direction only (12 instances): p, q and d are wave-uniform run-time values over fully
// unrolled predicated loops, so the register arrays are indexed by constants (no scratch).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sparkts_arima.h"
#include "arima_launch.hpp"
#include "row_tile.hpp"

namespace sts {

constexpr int kFxMaxOrder = 5;   // p, q <= 5
constexpr int kFxMaxD = 8;
using FxTile = RowTile<32>;
static_assert(kFxMaxOrder == kFastMaxOrder, "the dispatch in the runtime sends p, q <= kFastMaxOrder here");

// in_all and out_all may be the same rows (no __restrict__)
template <int MM, bool ADD>
__global__ __launch_bounds__(FxTile::kWave) void k_effects(const double *in_all, int64_t ld_in,
                                                           const double *__restrict__ coef_all, int k, double *out_all,
                                                           int64_t ld_out, int64_t N, int T, int p, int d, int q,
                                                           int I) {
    constexpr int kM = MM > 0 ? MM : 1;
    __shared__ FxTile::Lds tile;
    const int lane = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * FxTile::kWave;
    const int64_t sid = row0 + lane;
    const bool live = sid < N;
    // coefficients [c?, phi_1..phi_p, theta_1..theta_q] (ARIMA.scala:74-77); k == 0 reads nothing
    const double *cf = coef_all + (live ? sid : N - 1) * k;
    const double c0 = k > 0 ? cf[0] : 0.0;
    double phi[kM], th[kM];
#pragma unroll
    for (int j = 0; j < MM; ++j) {
        phi[j] = j < p ? cf[I + j] : 0.0;
        th[j] = j < q ? cf[I + p + j] : 0.0;
    }
    const double ic = (double)I * c0;                                  // intercept * coefficients(0) (:600)
    const double ia = I ? c0 : 0.0;
    double hist[kM], ma[kM];
#pragma unroll
    for (int j = 0; j < MM; ++j) { hist[j] = ia; ma[j] = 0.0; }
    double lv[kFxMaxD];                                                // Dp (remove) / Ip (add)
#pragma unroll
    for (int r = 0; r < kFxMaxD; ++r) lv[r] = 0.0;

    const unsigned long long mask = FxTile::rows_below(row0, N);
    FxTile::map(tile, in_all, ld_in, out_all, ld_out, row0, N, T, lane, mask, [&](int cb, int n) {
        const int ce = cb + n;
#pragma unroll 1
        for (int t = cb; t < ce; ++t) {
            const double v = tile[lane][t - cb];
            double x = v, w;
            if (!ADD) {
                // differencing column t (UnivariateTimeSeries.scala:384-405 pass r: out(t) = in(t) - in(t-1), t >= r)
#pragma unroll
                for (int r = 1; r <= kFxMaxD; ++r)
                    if (r <= d) {
                        const double nx = t < r ? x : x - lv[r - 1];
                        lv[r - 1] = x;
                        x = nx;
                    }
                w = x - ic;                                            // iterateARMA, op = -, ARIMA.scala:581-618
#pragma unroll
                for (int j = 0; j < MM; ++j)
                    if (j < p) w = w - hist[j] * phi[j];
#pragma unroll
                for (int j = 0; j < MM; ++j)
                    if (j < q) w = w - ma[j] * th[j];
            } else {
                w = v + ic;                                            // iterateARMA, op = +
#pragma unroll
                for (int j = 0; j < MM; ++j)
                    if (j < p) w = w + hist[j] * phi[j];
#pragma unroll
                for (int j = 0; j < MM; ++j)
                    if (j < q) w = w + ma[j] * th[j];
            }
            const double err = ADD ? v : w;                            // errors = the noise (:662) / dest itself (:640)
#pragma unroll
            for (int j = MM - 1; j >= 1; --j)                          // updateMAErrors (:544-554): smear
                if (j < q) ma[j] = ma[0];
            if (q > 0) ma[0] = err;
#pragma unroll
            for (int j = MM - 1; j >= 1; --j) hist[j] = hist[j - 1];
            if (MM > 0) hist[0] = ADD ? w : x;
            if (ADD) {
                // inverseDifferencesOfOrderD (:489-495): pass l over the row becomes the running sum lv[l-1]
#pragma unroll
                for (int l = kFxMaxD; l >= 1; --l)
                    if (l <= d) {
                        w = t < l ? w : w + lv[l - 1];
                        lv[l - 1] = w;
                    }
            }
            tile[lane][t - cb] = w;
        }
    });
}

template <bool ADD>
static int launch_effects_dir(const double *in, int64_t ld_in, const double *coef, int k, double *out, int64_t ld_out,
                              int64_t N, int T, int p, int d, int q, int I, hipStream_t s) {
    const dim3 grid((unsigned)((N + FxTile::kWave - 1) / FxTile::kWave)), block(FxTile::kWave);
    switch (p > q ? p : q) {
#define STS_FX_CASE(MM)                                                                                             \
    case MM:                                                                                                        \
        hipLaunchKernelGGL((k_effects<MM, ADD>), grid, block, 0, s, in, ld_in, coef, k, out, ld_out, N, T, p, d, q, \
                           I);                                                                                      \
        break;
    STS_FX_CASE(0) STS_FX_CASE(1) STS_FX_CASE(2) STS_FX_CASE(3) STS_FX_CASE(4) STS_FX_CASE(5)
#undef STS_FX_CASE
    }
    if (hipGetLastError() != hipSuccess) return ARIMA_E_DEVICE;
    return ARIMA_OK;
}

int launch_effects(const double *in, int64_t ld_in, const double *coef, int k, double *out, int64_t ld_out, int64_t N,
                   int T, int p, int d, int q, int I, int add, hipStream_t s) {
    if (N == 0 || T == 0) return ARIMA_OK;
    if (p < 0 || q < 0 || d < 0 || p > kFxMaxOrder || q > kFxMaxOrder || d > kFxMaxD) return ARIMA_E_UNSUPPORTED;
    if (T < d || k != I + p + q || ld_in < T || ld_out < T) return ARIMA_E_INVALID_ARG;
    return add ? launch_effects_dir<true>(in, ld_in, coef, k, out, ld_out, N, T, p, d, q, I, s)
               : launch_effects_dir<false>(in, ld_in, coef, k, out, ld_out, N, T, p, d, q, I, s);
}

}  // namespace sts
