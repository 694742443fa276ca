// arima_diag.hip — the residual diagnostics of the reference over a batch of rows, one launch:
//   acf   UnivariateTimeSeries.autocorr        (UnivariateTimeSeries.scala:70-96): lags 1 .. L
//   dw    TimeSeriesStatisticalTests.dwtest    (TimeSeriesStatisticalTests.scala:251-262)
//   lb    TimeSeriesStatisticalTests.lbtest    (:298-307): the statistic and its chi-squared p-value (arima_chisq.hpp)
// One lane per series, same operations in the same order as the reference (left folds, no fused multiply-add), so
// acf, dw and the Ljung-Box statistic are bit-identical to tests/diag_ref.py; the p-value is held to a tolerance
// (arima_chisq.hpp says why).
//
// autocorr recomputes, for every lag i, the means of ts[i..T) and ts[0..T-i) and then one loop of three centred sums.
// Lags are served in groups of W = kDgW. For its group a wave streams its 64 rows twice:
//   pass A  W suffix sums (the one of lag i starts at t = i: every mean is its own fold), one running prefix sum
//           snapshotted at t = T-i-1, and -- first group only -- the two Durbin-Watson folds;
//   pass B  the 3 W centred sums, with the last W values of the lagged operand in a register ring.
// Every further group of lags costs one more pass pair; any L < T works. The lagged operand of group g is the row
// delayed by g W steps: the first group takes it from the tile it already has, later groups stream a second tile.
// A call of at most W lags runs an instance of its own whose W is the smallest of 1, 2, 4, kDgW that holds them.
//
// Memory path: row_tile.hpp (RowTile<CH>::load and store). Register arrays are indexed by constants only: the loops
// over the lags of a group are fully unrolled and predicated on wave-uniform conditions (the lag count of the group and
// the step), and full tiles of full groups take an unpredicated path whose ring rotates by renaming over W steps.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sparkts_arima.h"
#include "arima_chisq.hpp"
#include "arima_launch.hpp"
#include "row_tile.hpp"

namespace sts {

constexpr int kDgWave = 64;

// Breeze `mean` of a slice (UnivariateTimeSeries.scala:77-78). Breeze is not vendored by the reference; this is the
// left-fold reading, sum += x from 0.0 then sum / m (unpinned). The other reading is the running-mean
// update mean += (x - mean) / cnt, finished by the identity; flip both functions together (cnt = elements so far,
// this one included).
__device__ __forceinline__ double dg_mean_step(double acc, double x, int cnt) {
    (void)cnt;
    return acc + x;
}
__device__ __forceinline__ double dg_mean_finish(double acc, int m) { return acc / (double)m; }

// MULTI = false: L <= W (one group; L == 0: Durbin-Watson alone); W is 1, 2, 4 (CH = 32) or kDgW (CH = 16), the
// smallest that holds L, so that short lag lists carry short register arrays and take the unpredicated path. These
// instances are held to two waves per SIMD (scratch 0 in all of them).
// MULTI = true: any L, groups of W = kDgW in turn inside the launch, a second tile for the delayed operand, CH = 16.
template <int CH, bool MULTI, int W>
__global__ __launch_bounds__(kDgWave) __attribute__((amdgpu_waves_per_eu(MULTI ? 1 : 2))) void k_diag(
    const double *__restrict__ rows, int64_t ld, int64_t N, int T, int L, double *__restrict__ acf_out,
    double *__restrict__ dw_out, double *__restrict__ lb_stat_out, double *__restrict__ lb_pvalue_out) {
    static_assert(W == kDgW || (!MULTI && kDgW % W == 0), "group width");
    using Tile = RowTile<CH>;                         // the memory path (row_tile.hpp)
    static_assert(CH % W == 0 && CH >= W, "tile width");
    __shared__ typename Tile::Lds tile;
    __shared__ double tile2[MULTI ? kDgWave : 1][CH + 1];
    const int lane = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kDgWave;
    const int64_t sid = row0 + lane;
    const bool live = sid < N;
    const int64_t Tl = T;

    const int nrows = (int)(N - row0 < kDgWave ? N - row0 : kDgWave);
    const unsigned long long mask = Tile::rows_below(row0, N);
    double pf[CH] = {}, pf2[MULTI ? CH : 1] = {};     // rows past N are never loaded: zero, and never consumed
    // one streaming pass over columns [cb0, T), RowTile::read with a start column and, for `two`, a second tile: the
    // row delayed by b columns. body(cb, n): the lane's row is tile[lane][0 .. n), columns cb .. cb + n
    auto stream = [&](int64_t cb0, bool two, int64_t b, auto &&body) {
        Tile::load(pf, rows, ld, row0, T, cb0, lane, mask);
        if constexpr (MULTI)
            if (two) Tile::load(pf2, rows, ld, row0, T, cb0 - b, lane, mask);
        for (int64_t cb = cb0; cb < Tl; cb += CH) {
            __syncthreads();                          // the last tile (or the acf flush) has been read
            Tile::store(tile, pf, lane);
            if constexpr (MULTI)
                if (two) Tile::store(tile2, pf2, lane);
            __syncthreads();
            if (cb + CH < Tl) {
                Tile::load(pf, rows, ld, row0, T, cb + CH, lane, mask);
                if constexpr (MULTI)
                    if (two) Tile::load(pf2, rows, ld, row0, T, cb + CH - b, lane, mask);
            }
            body(cb, (int)(cb + CH < Tl ? CH : Tl - cb));
        }
    };

    double lbsum = 0.0;                               // adjAutoCorrs.sum (:301-304), folded lag by lag
    const int ngroups = MULTI ? (L + W - 1) / W : 1;
    for (int g = 0; g < (ngroups > 0 ? ngroups : 1); ++g) {
        const int b = g * W;                          // this group serves lags b + 1 .. b + nl
        const int nl = L - b < W ? L - b : W;
        const bool first = g == 0;
        if (nl <= 0 && !(first && dw_out)) break;

        // ---- pass A: the 2 nl means (and dwtest) --------------------------------------------------------------
        double m1[W], m2[W];                          // suffix sums / prefix snapshots, then mean1 / mean2
#pragma unroll
        for (int k = 0; k < W; ++k) m1[k] = m2[k] = 0.0;
        double prefix = 0.0, prev = 0.0;
        double rs = 0.0, ds = 0.0;                    // dwtest's residsSum, diffsSum (first group)
        stream(0, false, 0, [&](int64_t cb, int n) {
            // no lag of the group starts or snapshots inside the tile: every suffix sum takes every element
            const bool steady = nl == W && cb >= (int64_t)b + W && cb + n <= Tl - 1 - b - W;
            if (steady) {                             // cb > 0 here: dwtest is past its first element
#pragma unroll 4
                for (int c = 0; c < n; ++c) {
                    const double x = tile[lane][c];
                    prefix = dg_mean_step(prefix, x, (int)cb + c + 1);
#pragma unroll
                    for (int k = 0; k < W; ++k) m1[k] = dg_mean_step(m1[k], x, (int)cb + c - b - k);
                    if (first) {
                        rs += x * x;
                        const double diff = x - prev;
                        ds += diff * diff;
                        prev = x;
                    }
                }
                return;
            }
#pragma unroll 1
            for (int c = 0; c < n; ++c) {
                const int64_t t = cb + c;
                const double x = tile[lane][c];
                prefix = dg_mean_step(prefix, x, (int)t + 1);
                const int64_t tb = t - b - 1;         // lag b + 1 + k has started iff tb >= k
                const int64_t sn = Tl - 2 - b - t;    // ... and takes its snapshot at t = T - 1 - (b + 1 + k)
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    if (k < nl && tb >= k) m1[k] = dg_mean_step(m1[k], x, (int)(tb - k) + 1);
                    if (k < nl && sn == k) m2[k] = prefix;
                }
                if (first) {                          // dwtest (:251-262)
                    if (t == 0) {
                        rs = x * x;
                    } else {
                        rs += x * x;
                        const double diff = x - prev;
                        ds += diff * diff;
                    }
                    prev = x;
                }
            }
        });
        if (first && dw_out && live) dw_out[sid] = ds / rs;   // here, so that the two folds are dead in pass B
        if (nl <= 0) break;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const int m = T - (b + 1 + k);
            m1[k] = dg_mean_finish(m1[k], m);
            m2[k] = dg_mean_finish(m2[k], m);
        }

        // ---- pass B: variance1, variance2, covariance of every lag of the group (:79-90) ---------------------
        double v1[W], v2[W], cv[W], ring[W];          // ring[k] = x[t - b - 1 - k], the operand of lag b + 1 + k
#pragma unroll
        for (int k = 0; k < W; ++k) v1[k] = v2[k] = cv[k] = ring[k] = 0.0;
        const bool two = MULTI && b > 0;
        stream(MULTI ? (int64_t)(b / CH) * CH : 0, two, b, [&](int64_t cb, int n) {
            if (nl == W && n == CH && cb >= (int64_t)b + W) {
                // every lag is live at every step of the tile; ring slot (k - s) mod W holds lag k's operand at
                // step s of a block of W, and slot W - 1 - s takes the new value
#pragma unroll 1
                for (int c0 = 0; c0 < CH; c0 += W) {
#pragma unroll
                    for (int s = 0; s < W; ++s) {
                        const double x = tile[lane][c0 + s];
                        const double xu = two ? tile2[lane][c0 + s] : x;
#pragma unroll
                        for (int k = 0; k < W; ++k) {
                            const double d1 = x - m1[k];
                            const double d2 = ring[(k - s + W) % W] - m2[k];
                            v1[k] += d1 * d1;
                            v2[k] += d2 * d2;
                            cv[k] += d1 * d2;
                        }
                        ring[W - 1 - s] = xu;
                        // one step's temporaries at a time: with the steps interleaved the 8-lag instance
                        // does not fit the 256 registers of two waves per SIMD
                        if constexpr (W == kDgW) __builtin_amdgcn_sched_barrier(0);
                    }
                }
                return;
            }
#pragma unroll 1
            for (int c = 0; c < n; ++c) {
                const int64_t tb = cb + c - b - 1;
                const double x = tile[lane][c];
                const double xu = two ? tile2[lane][c] : x;
#pragma unroll
                for (int k = 0; k < W; ++k)
                    if (k < nl && tb >= k) {
                        const double d1 = x - m1[k];
                        const double d2 = ring[k] - m2[k];
                        v1[k] += d1 * d1;
                        v2[k] += d2 * d2;
                        cv[k] += d1 * d2;
                    }
#pragma unroll
                for (int k = W - 1; k >= 1; --k) ring[k] = ring[k - 1];
                ring[0] = xu;
            }
        });

        // ---- the group's correlations (:92) and their Ljung-Box terms (:301-303) ---------------------------------
        __syncthreads();                              // the last tile has been read
#pragma unroll
        for (int k = 0; k < W; ++k)
            if (k < nl) {
                const double corr = cv[k] / (sqrt(v1[k]) * sqrt(v2[k]));
                lbsum += (corr * corr) / (double)(T - (b + k) - 1);
                tile[lane][k] = corr;
            }
        if (acf_out) {                                // coalesced row segments of nl correlations
            __syncthreads();
            constexpr int FW = kDgW, FR = kDgWave / kDgW;     // the flush: FR rows x FW lags per store instruction
            const int c = lane % FW, rr = lane / FW;
            if (c < nl) {
                double *dst = acf_out + (row0 + rr) * L + b + c;
                asm volatile("" : "+v"(dst));         // as in RowTile::load
#pragma unroll
                for (int j = 0; j < FW; ++j)
                    if (rr < nrows - j * FR) dst[(int64_t)j * FR * L] = tile[j * FR + rr][c];
            }
        }
    }
    if (!live) return;
    if (lb_stat_out || lb_pvalue_out) {
        // n * (n + 2) is an Int product in the reference (:304): it wraps for n >= 46340
        const int32_t nn = (int32_t)((uint32_t)T * ((uint32_t)T + 2u));
        const double stat = (double)nn * lbsum;
        if (lb_stat_out) lb_stat_out[sid] = stat;
        if (lb_pvalue_out) lb_pvalue_out[sid] = chisq_upper_tail(L, stat);
    }
}

int launch_diag(const double *rows, int64_t ld, int64_t N, int T, int max_lag, double *acf_out, double *dw_out,
                double *lb_stat_out, double *lb_pvalue_out, hipStream_t s) {
    if (N == 0 || T == 0) return ARIMA_OK;
    if (!acf_out && !dw_out && !lb_stat_out && !lb_pvalue_out) return ARIMA_OK;
    const bool lags = acf_out || lb_stat_out || lb_pvalue_out;
    if (N < 0 || T < 0 || ld < T || (lags && (max_lag < 1 || max_lag > T - 1))) return ARIMA_E_INVALID_ARG;
    const int L = lags ? max_lag : 0;
    const dim3 grid((unsigned)((N + kDgWave - 1) / kDgWave)), block(kDgWave);
#define STS_DG_LAUNCH(CH, MULTI, W)                                                                             \
    hipLaunchKernelGGL((k_diag<CH, MULTI, W>), grid, block, 0, s, rows, ld, N, T, L, acf_out, dw_out, lb_stat_out, \
                       lb_pvalue_out)
    if (L <= 1)
        STS_DG_LAUNCH(32, false, 1);
    else if (L <= 2)
        STS_DG_LAUNCH(32, false, 2);
    else if (L <= 4)
        STS_DG_LAUNCH(32, false, 4);
    else if (L <= kDgW)
        STS_DG_LAUNCH(16, false, kDgW);   // 32-wide tiles would spill at two waves per SIMD
    else
        STS_DG_LAUNCH(16, true, kDgW);
#undef STS_DG_LAUNCH
    if (hipGetLastError() != hipSuccess) return ARIMA_E_DEVICE;
    return ARIMA_OK;
}

}  // namespace sts
