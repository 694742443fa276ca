// arima_regress.hip — the reference's regressions over a design matrix that is not made only of a series' own lags:
//   arx   AutoregressionX.fitModel, ARXModel.predict   (AutoregressionX.scala:48-130, Lag.scala:33-118)
//   bg    TimeSeriesStatisticalTests.bgtest            (TimeSeriesStatisticalTests.scala:276-288)
//   bp    TimeSeriesStatisticalTests.bptest            (:320-329)
//   co    RegressionARIMA.fitCochraneOrcutt            (RegressionARIMA.scala:83-176)
// All four are commons-math3 3.4.1 OLSMultipleLinearRegression: QRDecomposition at threshold 0 and its Solver
// (SURVEY.md Appendix A-5), the tests with calculateRSquared on top. One lane per series, the reference's operations
// in its order (left folds, no fused multiply-add): coefficients, fitted values and the statistics are bit-identical
// to tests/regress_ref.py (co: tests/regarima_ref.py); the p-values go through arima_chisq.hpp and are held to its
// tolerance.
//
// The design is written once into a workspace the handle owns (RgDesign::col names every column as a window of a
// source row), laid out so that a wave's accesses are contiguous: element (series 64 b + lane, column c, row r) at
// ws[((b (C + 1) + c) R + r) 64 + lane], column C the response. The QR then runs literally, in place, per lane; its
// state beyond the workspace is rDiag[C] (LDS, one column per lane) and scalars. The tests assemble a second time:
// the QR has destroyed the design that calculateRSquared multiplies by beta. Cochrane-Orcutt runs up to maxIter + 1 QRs
// per series inside one kernel, each on a working design it rebuilds from a pristine copy of y and X in the same layout
// (k_cochrane_orcutt). Every index into the workspace is 64-bit.
//
// Memory path of the per-series sources: row_tile.hpp. A shared regressor matrix is read directly (every lane reads
// the same address).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sparkts_arima.h"
#include "arima_chisq.hpp"
#include "arima_launch.hpp"
#include "row_tile.hpp"

namespace sts {

constexpr int kRgWave = 64;
constexpr int kRgCH = 32;          // tile width of the assembly
constexpr int kRgPredCH = 16;      // rows of ARXModel.predict per flush

// KIND: the row generator (kRgArx, kRgBg, kRgBp, kRgCo); RgDesign::col with the kind a constant
template <int KIND>
__global__ __launch_bounds__(kRgWave) void k_regress_assemble(RgDesign dd, RgSrc src, int64_t N,
                                                              double *__restrict__ ws) {
    using Tile = RowTile<kRgCH>;
    __shared__ typename Tile::Lds tile;
    RgDesign d = dd;
    d.kind = KIND;
    const int lane = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kRgWave;
    const bool live = row0 + lane < N;
    const unsigned long long mask = Tile::rows_below(row0, N);
    const int R = d.rows(), C = d.cols();
    const int64_t cstride = (int64_t)R * kRgWave;
    double *q = ws + (int64_t)blockIdx.x * (C + 1) * cstride + lane;

    // every column that is a window of the streamed row `which`, tile by tile
    auto stream = [&](int which, const double *in, int64_t ld) {
        Tile::read(tile, in, ld, row0, d.T, lane, mask, [&](int cb, int n) {
            if (!live) return;
            for (int c = 0; c <= C; ++c) {
                const RgCol col = d.col(c);
                if (col.src != which) continue;
                double *dst = q + c * cstride;
                const int i0 = col.off > cb ? col.off - cb : 0;               // design rows [0, R) inside this tile
                const int i1 = col.off + R - cb < n ? col.off + R - cb : n;
                for (int i = i0; i < i1; ++i) {
                    const double v = tile[lane][i];
                    dst[(int64_t)(cb + i - col.off) * kRgWave] = col.sq ? v * v : v;
                }
            }
        });
    };

    stream(kRgSelf, src.y, src.ld);
    for (int j = 0; j < d.k; ++j) {
        if (src.xs != 0) {
            stream(j, src.x + (int64_t)j * d.T, src.xs);
            continue;
        }
        if (!live) continue;
        const double *xj = src.x + (int64_t)j * d.T;
        for (int c = 0; c < C; ++c) {
            const RgCol col = d.col(c);
            if (col.src != j) continue;
            double *dst = q + c * cstride;
            for (int r = 0; r < R; ++r) dst[(int64_t)r * kRgWave] = xj[col.off + r];
        }
    }
    if (live && d.icpt)
        for (int r = 0; r < R; ++r) q[(int64_t)r * kRgWave] = 1.0;            // column 0
}

// QRDecomposition.decompose (performHouseholderReflection per minor), Solver.isNonSingular at threshold 0, then
// Solver.solve on the response column: y = Q^T y minor by minor, back-substitution from the last row up. One lane's
// design in place: q is its element (column 0, row 0), columns cstride apart, rows kRgWave apart, column C the
// response; rdiag its rDiag[C] (LDS, kRgWave apart). False: singular, nothing solved. True: beta is rows 0 .. C-1 of
// the response column. Both k_regress_qr and k_cochrane_orcutt run this.
__device__ __forceinline__ bool rg_qr_solve(double *q, int64_t cstride, int R, int C, double *rdiag) {
    for (int minor = 0; minor < C; ++minor) {
        double *qm = q + minor * cstride;
        double norm = 0.0;
#pragma unroll 8
        for (int row = minor; row < R; ++row) {
            const double c = qm[(int64_t)row * kRgWave];
            norm = norm + c * c;
        }
        const double qmm0 = qm[(int64_t)minor * kRgWave];
        const double a = qmm0 > 0 ? -sqrt(norm) : sqrt(norm);
        rdiag[minor * kRgWave] = a;
        if (a != 0.0) {
            const double qmm = qmm0 - a;
            qm[(int64_t)minor * kRgWave] = qmm;
            const double den = a * qmm;
            for (int col = minor + 1; col < C; ++col) {
                double *qc = q + col * cstride;
                double alpha = 0.0;
#pragma unroll 8
                for (int row = minor; row < R; ++row)
                    alpha = alpha - qc[(int64_t)row * kRgWave] * qm[(int64_t)row * kRgWave];
                alpha = alpha / den;
#pragma unroll 8
                for (int row = minor; row < R; ++row)
                    qc[(int64_t)row * kRgWave] = qc[(int64_t)row * kRgWave] - alpha * qm[(int64_t)row * kRgWave];
            }
        }
    }

    bool singular = false;
    for (int i = 0; i < C; ++i) singular = singular || fabs(rdiag[i * kRgWave]) <= 0.0;
    if (singular) return false;
    double *yv = q + C * cstride;
    for (int minor = 0; minor < C; ++minor) {
        const double *qm = q + minor * cstride;
        double dot = 0.0;
#pragma unroll 8
        for (int row = minor; row < R; ++row) dot = dot + yv[(int64_t)row * kRgWave] * qm[(int64_t)row * kRgWave];
        dot = dot / (rdiag[minor * kRgWave] * qm[(int64_t)minor * kRgWave]);
#pragma unroll 8
        for (int row = minor; row < R; ++row)
            yv[(int64_t)row * kRgWave] = yv[(int64_t)row * kRgWave] + dot * qm[(int64_t)row * kRgWave];
    }
    for (int row = C - 1; row >= 0; --row) {
        const double y_row = yv[(int64_t)row * kRgWave] / rdiag[row * kRgWave];
        yv[(int64_t)row * kRgWave] = y_row;
        const double *qr = q + row * cstride;
        for (int i = 0; i < row; ++i)
            yv[(int64_t)i * kRgWave] = yv[(int64_t)i * kRgWave] - y_row * qr[(int64_t)i * kRgWave];
    }
    return true;
}

// At most 4 waves per SIMD: the folds are bound by the latency of their strided loads, and only under a register
// budget above the 64 of 8 waves does the scheduler issue the 16 loads of an unrolled fold together, not pair by pair
// (65 536 x 1024, ARX(2, 1), k = 2: 21.9 ms against 34.7 ms at the default).
__global__ __launch_bounds__(kRgWave) __attribute__((amdgpu_waves_per_eu(1, 4)))
void k_regress_qr(double *__restrict__ ws, int64_t N, int R, int C, double *__restrict__ beta_out, int ldb, int boff,
                  int c_zero, int32_t *__restrict__ status_out) {
    extern __shared__ __attribute__((aligned(16))) double rg_lds[];          // rDiag[C][64]
    const int lane = (int)threadIdx.x;
    const int64_t sid = (int64_t)blockIdx.x * kRgWave + lane;
    if (sid >= N) return;                                                     // no barrier below
    const int64_t cstride = (int64_t)R * kRgWave;
    double *q = ws + (int64_t)blockIdx.x * (C + 1) * cstride + lane;
    double *out = beta_out + sid * ldb;
    if (!rg_qr_solve(q, cstride, R, C, rg_lds + lane)) {
        status_out[sid] = ARIMA_ST_SINGULAR;
        for (int i = 0; i < boff + C; ++i) out[i] = __builtin_nan("");
        return;
    }
    const double *yv = q + C * cstride;
    for (int row = 0; row < C; ++row) out[boff + row] = yv[(int64_t)row * kRgWave];
    if (c_zero) out[0] = 0.0;                                                 // noIntercept: c = 0.0
    status_out[sid] = ARIMA_ST_OK;
}

// calculateTotalSumOfSquares with an intercept: commons-math3 3.4.1 SecondMoment.evaluate over the n values at
// y[0], y[stride], ..., the running update n++; dev = y - m1; nDev = dev / n; m1 += nDev;
// m2 += ((double) n - 1) * dev * nDev, associated left to right. Commons is not vendored by the reference: an unpinned
// reading; flip it here and in second_moment (tests/regress_ref.py) together.
__device__ __forceinline__ double rg_second_moment(const double *y, int64_t stride, int n) {
    double m1 = 0.0, m2 = 0.0;
    for (int i = 0; i < n; ++i) {
        const double cnt = (double)(i + 1);
        const double dev = y[i * stride] - m1;
        const double n_dev = dev / cnt;
        m1 += n_dev;
        m2 += (cnt - 1.0) * dev * n_dev;
    }
    return m2;
}

// calculateRSquared = 1 - RSS / TSS on a freshly assembled design: the fitted value of a row is the left fold over all
// C columns, the ones column included (Array2DRowRealMatrix.operate); RSS the left fold of res * res
__global__ __launch_bounds__(kRgWave) void k_regress_r2(const double *__restrict__ ws, const double *__restrict__ beta,
                                                        const int32_t *__restrict__ status, int64_t N, int R, int C,
                                                        int nobs, int df, double *__restrict__ stat_out,
                                                        double *__restrict__ pvalue_out) {
    extern __shared__ __attribute__((aligned(16))) double rg_lds[];          // beta[C][64]
    const int lane = (int)threadIdx.x;
    const int64_t sid = (int64_t)blockIdx.x * kRgWave + lane;
    if (sid >= N) return;
    if (status[sid] != ARIMA_ST_OK) {
        stat_out[sid] = __builtin_nan("");
        pvalue_out[sid] = __builtin_nan("");
        return;
    }
    const int64_t cstride = (int64_t)R * kRgWave;
    const double *q = ws + (int64_t)blockIdx.x * (C + 1) * cstride + lane;
    double *b = rg_lds + lane;
    for (int c = 0; c < C; ++c) b[c * kRgWave] = beta[sid * C + c];
    const double *y = q + C * cstride;
    double rss = 0.0;
    for (int r = 0; r < R; ++r) {
        const double *x = q + (int64_t)r * kRgWave;
        double sum = 0.0;
#pragma unroll 4
        for (int c = 0; c < C; ++c) sum += x[c * cstride] * b[c * kRgWave];
        const double res = y[(int64_t)r * kRgWave] - sum;
        rss += res * res;
    }
    const double tss = rg_second_moment(y, kRgWave, R);
    const double stat = (double)nobs * (1.0 - rss / tss);
    stat_out[sid] = stat;
    pvalue_out[sid] = chisq_upper_tail(df, stat);
}

// ARXModel.predict (:117-130): results(r) = c, then += value * coefficients(col) in column order. A lane keeps
// kRgPredCH rows' sums and takes the columns in order, so every sum sees its terms in the reference's order; the rows
// leave through the row tile as coalesced segments.
__global__ __launch_bounds__(kRgWave) void k_arx_predict(RgDesign dd, RgSrc src, const double *__restrict__ coef,
                                                         double *__restrict__ out, int64_t ld_out, int64_t N) {
    using Tile = RowTile<kRgPredCH>;
    __shared__ typename Tile::Lds tile;
    RgDesign d = dd;
    d.kind = kRgArx;
    d.icpt = 0;                                    // columns 0 .. K-1 are the predictors
    const int lane = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kRgWave;
    const int64_t sid = row0 + lane;
    const bool live = sid < N;
    const int R = d.rows(), K = d.cols();
    const double *cf = coef + (live ? sid : 0) * (int64_t)(1 + K);
    const double *ys = src.y + (live ? sid : 0) * src.ld;
    const double *xs = src.x ? src.x + (live ? sid : 0) * src.xs : nullptr;   // no regressors: never read
    for (int r0 = 0; r0 < R; r0 += kRgPredCH) {
        const int n = R - r0 < kRgPredCH ? R - r0 : kRgPredCH;
        double acc[kRgPredCH];
        if (live) {
            const double c0 = cf[0];
#pragma unroll
            for (int i = 0; i < kRgPredCH; ++i) acc[i] = c0;
            for (int c = 0; c < K; ++c) {
                const RgCol col = d.col(c);
                const double w = cf[1 + c];
                const double *v = (col.src == kRgSelf ? ys : xs + (int64_t)col.src * d.T) + col.off + r0;
#pragma unroll
                for (int i = 0; i < kRgPredCH; ++i)
                    if (i < n) acc[i] += v[i] * w;
            }
        }
        __syncthreads();                           // the last flush has read the tile
        if (live) {
#pragma unroll
            for (int i = 0; i < kRgPredCH; ++i) tile[lane][i] = acc[i];
        }
        __syncthreads();
        Tile::flush(tile, out, ld_out, row0, N, R, r0, lane);
    }
}

// RegressionARIMA.isAutoCorrelated of a Durbin-Watson statistic: the bounds are the reference's double expressions;
// a NaN statistic compares false twice (not autocorrelated)
__device__ __forceinline__ bool co_autocorrelated(double diffs, double resids) {
    const double margin = 0.05;
    const double dw = diffs / resids;
    return dw <= (2 - margin) || dw >= (2 + margin);
}

// RegressionARIMA.fitCochraneOrcutt (RegressionARIMA.scala:83-160), the whole loop of a series in its lane. ps: the
// pristine copy k_regress_assemble<kRgCo> wrote, columns x_0 .. x_{k-1} then y over T rows; wk: the working design
// (ones, k columns, response; column stride T rows whatever the row count), rebuilt from ps before each QR, which
// destroys it. Lanes leave the loop at different iterations: nothing below is a cross-lane operation or a barrier, a
// lane that is done only waits for its wave.
// One pass over ps after each solve makes everything else, in the reference's order:
//   step 1   res = estimateResiduals (left fold over all columns, the ones column first): its dwtest sums and the
//            SimpleRegression(false) sums of the pairs (res(i), res(i + 1))
//   loop     tres = estimateResiduals of the transformed regression, Xdash recomputed as the design build computed it
//            (product, then difference): its dwtest sums; res(t) = y(t) - (dgemv + beta(0) / (1 - rho)): the pair sums
// SimpleRegression's sums (sumXX += x * x; sumXY += x * y) and F2J dgemv('N')'s order (sum = 0.0; sum += beta(1 + c) *
// X(t, c) in column order, the intercept added last) are unpinned readings: flip them here and in
// tests/regarima_ref.py together.
__global__ __launch_bounds__(kRgWave) void k_cochrane_orcutt(const double *__restrict__ ps, double *__restrict__ wk,
                                                             int64_t N, int T, int k, int max_iter,
                                                             double *__restrict__ coef_out,
                                                             double *__restrict__ rho_out,
                                                             int32_t *__restrict__ n_iter_out,
                                                             int32_t *__restrict__ status_out) {
    extern __shared__ __attribute__((aligned(16))) double rg_lds[];          // rDiag[C][64], beta[C][64]
    const int lane = (int)threadIdx.x;
    const int64_t sid = (int64_t)blockIdx.x * kRgWave + lane;
    if (sid >= N) return;                                                     // no barrier below
    const int C = k + 1;
    const int64_t cstride = (int64_t)T * kRgWave;
    const double *p = ps + (int64_t)blockIdx.x * (k + 1) * cstride + lane;
    const double *py = p + k * cstride;
    double *q = wk + (int64_t)blockIdx.x * (C + 1) * cstride + lane;
    double *rdiag = rg_lds + lane;
    double *b = rg_lds + C * kRgWave + lane;
    const double nan = __builtin_nan("");

    int32_t status = ARIMA_ST_OK;
    int iter = 0;
    double rho = 0.0, rho_before = 0.0;            // rhos(iter - 1), rhos(iter - 2); rhos is zero-filled
    double sxx = 0.0, sxy = 0.0;                   // of the pairs of the current origRegResiduals
    bool finished;

    // Step 1: OLS of y on [1, X] over T rows (the entry point has refused T == 0 and k + 1 > T)
    for (int r = 0; r < T; ++r) {
        const int64_t o = (int64_t)r * kRgWave;
        q[o] = 1.0;
        for (int c = 0; c < k; ++c) q[(1 + c) * cstride + o] = p[c * cstride + o];
        q[C * cstride + o] = py[o];
    }
    if (!rg_qr_solve(q, cstride, T, C, rdiag)) {
        status = ARIMA_ST_SINGULAR;
        finished = true;
    } else {
        for (int c = 0; c < C; ++c) b[c * kRgWave] = q[C * cstride + (int64_t)c * kRgWave];
        double resids = 0.0, diffs = 0.0, before = 0.0;
        for (int t = 0; t < T; ++t) {
            const int64_t o = (int64_t)t * kRgWave;
            double sum = 0.0;
            sum += 1.0 * b[0];
            for (int c = 0; c < k; ++c) sum += p[c * cstride + o] * b[(1 + c) * kRgWave];
            const double res = py[o] - sum;
            if (t == 0) {
                resids = res * res;
            } else {
                resids += res * res;
                const double diff = res - before;
                diffs += diff * diff;
                sxx += before * before;
                sxy += before * res;
            }
            before = res;
        }
        finished = !co_autocorrelated(diffs, resids);
    }

    while (!finished) {
        // (a) SimpleRegression(false).getSlope over T - 1 pairs
        rho_before = rho;
        rho = (T - 1 < 2 || fabs(sxx) < 10 * 4.9406564584124654e-324) ? nan : sxy / sxx;
        // (b), (c) OLS of Ydash on [1, Xdash] over T - 1 rows: validateSampleData first
        const int R = T - 1;
        if (R == 0) status = ARIMA_ST_NO_DATA;
        else if (k + 1 > R) status = ARIMA_ST_NOT_ENOUGH_DATA;
        if (status != ARIMA_ST_OK) break;
        for (int r = 0; r < R; ++r) {
            const int64_t o = (int64_t)r * kRgWave, o1 = o + kRgWave;
            q[o] = 1.0;
            for (int c = 0; c < k; ++c) q[(1 + c) * cstride + o] = p[c * cstride + o1] - p[c * cstride + o] * rho;
            q[C * cstride + o] = py[o1] - py[o] * rho;
        }
        if (!rg_qr_solve(q, cstride, R, C, rdiag)) {
            status = ARIMA_ST_SINGULAR;
            break;
        }
        for (int c = 0; c < C; ++c) b[c * kRgWave] = q[C * cstride + (int64_t)c * kRgWave];
        const double b0t = b[0];                   // estimateResiduals solves again: the transformed intercept
        const double b0 = b0t / (1 - rho);         // (d)
        b[0] = b0;
        double resids = 0.0, diffs = 0.0, tbefore = 0.0, before = 0.0;
        sxx = 0.0;
        sxy = 0.0;
        for (int t = 0; t < T; ++t) {
            const int64_t o = (int64_t)t * kRgWave;
            if (t >= 1) {
                double sum = 0.0;
                sum += 1.0 * b0t;
                for (int c = 0; c < k; ++c) {
                    const double xd = p[c * cstride + o] - p[c * cstride + o - kRgWave] * rho;
                    sum += xd * b[(1 + c) * kRgWave];
                }
                const double tres = (py[o] - py[o - kRgWave] * rho) - sum;
                if (t == 1) {
                    resids = tres * tres;
                } else {
                    resids += tres * tres;
                    const double diff = tres - tbefore;
                    diffs += diff * diff;
                }
                tbefore = tres;
            }
            double sum = 0.0;                      // (e)
            for (int c = 0; c < k; ++c) sum += b[(1 + c) * kRgWave] * p[c * cstride + o];
            const double res = py[o] - (sum + b0);
            if (t >= 1) {
                sxx += before * before;
                sxy += before * res;
            }
            before = res;
        }
        iter += 1;                                 // (f)
        finished = !co_autocorrelated(diffs, resids) || iter >= max_iter ||
                   (iter >= 2 && fabs(rho - rho_before) <= 0.001);
    }

    double *out = coef_out + sid * C;
    const bool ok = status == ARIMA_ST_OK;
    for (int c = 0; c < C; ++c) out[c] = ok ? b[c * kRgWave] : nan;
    rho_out[sid] = ok ? rho : nan;                 // rhos(max(0, iter - 1)): 0.0 when nothing iterated
    if (n_iter_out) n_iter_out[sid] = iter;
    status_out[sid] = status;
}

__global__ void k_regress_refuse(int64_t N, int32_t code, int32_t *__restrict__ status_out, double *__restrict__ out0,
                                 int n0, double *__restrict__ out1, int n1) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    status_out[i] = code;
    for (int j = 0; j < n0; ++j) out0[i * n0 + j] = __builtin_nan("");
    for (int j = 0; j < n1; ++j) out1[i * n1 + j] = __builtin_nan("");
}

static bool rg_shape_ok(int R, int C) { return R >= 1 && C >= 1 && C <= kRgMaxCols; }
static dim3 rg_grid(int64_t N) { return dim3((unsigned)((N + kRgWave - 1) / kRgWave)); }

int launch_regress_assemble(const RgDesign &d, const RgSrc &src, int64_t N, double *ws, hipStream_t s) {
    if (N == 0) return ARIMA_OK;
    if (N < 0 || !rg_shape_ok(d.rows(), d.cols()) || !ws || !src.y || src.ld < d.T || (d.k > 0 && !src.x) ||
        (src.xs != 0 && src.xs < (int64_t)d.k * d.T))
        return ARIMA_E_INVALID_ARG;
    const dim3 grid = rg_grid(N), block(kRgWave);
    if (d.kind == kRgArx)
        hipLaunchKernelGGL((k_regress_assemble<kRgArx>), grid, block, 0, s, d, src, N, ws);
    else if (d.kind == kRgBg)
        hipLaunchKernelGGL((k_regress_assemble<kRgBg>), grid, block, 0, s, d, src, N, ws);
    else if (d.kind == kRgCo)
        hipLaunchKernelGGL((k_regress_assemble<kRgCo>), grid, block, 0, s, d, src, N, ws);
    else
        hipLaunchKernelGGL((k_regress_assemble<kRgBp>), grid, block, 0, s, d, src, N, ws);
    return hipGetLastError() == hipSuccess ? ARIMA_OK : ARIMA_E_DEVICE;
}

int launch_regress_qr(double *ws, int64_t N, int R, int C, double *beta_out, int ldb, int boff, int c_zero,
                      int32_t *status_out, hipStream_t s) {
    if (N == 0) return ARIMA_OK;
    if (N < 0 || !rg_shape_ok(R, C) || !ws || !beta_out || !status_out || ldb < boff + C) return ARIMA_E_INVALID_ARG;
    hipLaunchKernelGGL(k_regress_qr, rg_grid(N), dim3(kRgWave), (size_t)C * kRgWave * sizeof(double), s, ws, N, R, C,
                       beta_out, ldb, boff, c_zero, status_out);
    return hipGetLastError() == hipSuccess ? ARIMA_OK : ARIMA_E_DEVICE;
}

int launch_regress_r2(const double *ws, const double *beta, const int32_t *status, int64_t N, int R, int C, int nobs,
                      int df, double *stat_out, double *pvalue_out, hipStream_t s) {
    if (N == 0) return ARIMA_OK;
    if (N < 0 || !rg_shape_ok(R, C) || !ws || !beta || !status || !stat_out || !pvalue_out || df < 1)
        return ARIMA_E_INVALID_ARG;
    hipLaunchKernelGGL(k_regress_r2, rg_grid(N), dim3(kRgWave), (size_t)C * kRgWave * sizeof(double), s, ws, beta,
                       status, N, R, C, nobs, df, stat_out, pvalue_out);
    return hipGetLastError() == hipSuccess ? ARIMA_OK : ARIMA_E_DEVICE;
}

int launch_arx_predict(const RgDesign &d, const RgSrc &src, const double *coef, double *out, int64_t ld_out, int64_t N,
                       hipStream_t s) {
    if (N == 0 || d.rows() == 0) return ARIMA_OK;
    if (N < 0 || d.rows() < 0 || d.num_pred() > kRgMaxCols || !coef || !out || ld_out < d.rows() || !src.y ||
        src.ld < d.T || (d.k > 0 && !src.x) || (src.xs != 0 && src.xs < (int64_t)d.k * d.T))
        return ARIMA_E_INVALID_ARG;
    hipLaunchKernelGGL(k_arx_predict, rg_grid(N), dim3(kRgWave), 0, s, d, src, coef, out, ld_out, N);
    return hipGetLastError() == hipSuccess ? ARIMA_OK : ARIMA_E_DEVICE;
}

int launch_cochrane_orcutt(const double *ps, double *wk, int64_t N, int T, int k, int max_iter, double *coef_out,
                           double *rho_out, int32_t *n_iter_out, int32_t *status_out, hipStream_t s) {
    if (N == 0) return ARIMA_OK;
    if (N < 0 || k < 1 || !rg_shape_ok(T, k + 1) || k + 1 > T || max_iter < 1 || !ps || !wk || !coef_out || !rho_out ||
        !status_out)
        return ARIMA_E_INVALID_ARG;
    hipLaunchKernelGGL(k_cochrane_orcutt, rg_grid(N), dim3(kRgWave), (size_t)2 * (k + 1) * kRgWave * sizeof(double), s,
                       ps, wk, N, T, k, max_iter, coef_out, rho_out, n_iter_out, status_out);
    return hipGetLastError() == hipSuccess ? ARIMA_OK : ARIMA_E_DEVICE;
}

int launch_regress_refuse(int64_t N, int32_t status, int32_t *status_out, double *out0, int n0, double *out1, int n1,
                          hipStream_t s) {
    if (N <= 0) return N == 0 ? ARIMA_OK : ARIMA_E_INVALID_ARG;
    if (!status_out) return ARIMA_E_INVALID_ARG;
    hipLaunchKernelGGL(k_regress_refuse, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, N, status, status_out,
                       out0, out0 ? n0 : 0, out1, out1 ? n1 : 0);
    return hipGetLastError() == hipSuccess ? ARIMA_OK : ARIMA_E_DEVICE;
}

}  // namespace sts
