// arima_models.hip — the small model families of spark-ts over a batch, one lane per series:
//   EWMA        EWMA.fitModel (EWMA.scala:45-69), EWMAModel.sse / gradient and its TimeSeriesModel pair (:81-143)
//   GARCH(1,1)  GARCH.fitModel (GARCH.scala:33-53), GARCHModel.logLikelihood / gradient and its pair (:82-162)
//   ARGARCH     ARGARCH.fitModel (GARCH.scala:63-69) and ARGARCHModel's pair (:205-236)
//   AR(p)       ARModel's pair (Autoregression.scala:60-90), p <= 20 at run time
//   sample      GARCHModel.sample / ARGARCHModel.sample (GARCH.scala:164-185, 238-259) from the caller's normals
// Both fits run commons-math3's Fletcher-Reeves NonLinearConjugateGradientOptimizer with its default LineSearch under
// SimpleValueChecker(1e-6, 1e-6), MaxIter(10000), MaxEval(10000): cg_small.hpp restates it as a per-series state machine
// (EWMA minimises sse; GARCH passes no GoalType, so commons maximises the log-likelihood). The objectives and the pairs
// are the one-pass recursions of model_pass.hpp, the reference's operations in its order; tests/smallfit_ref.py is the
// CPU restatement the results equal bit for bit.
//
// The reference's gradient-order quirk is reproduced, not repaired: GARCHModel.gradient returns (alpha, beta, omega)
// halves while the optimizer's parameters are (omega, alpha, beta), so omega moves along alpha's derivative, alpha along
// beta's and beta along omega's. A drop-in returns what spark-ts returns.
//
// k_model_fit<Model>: one wave per 64 series, wave-synchronous rounds. Every live lane has one posted point; one joint
// pass over the wave's rows computes objective and gradient at each lane's point; each lane advances its machine;
// finished lanes are masked; the wave leaves when all are done. Rows stream through row_tile.hpp (RowTile<32>::read);
// rows of finished lanes and rows past N are not read (their tile entries are never consumed). Everything carried
// across tile boundaries is in registers (Model::Pass). No stragglers are moved and no row stays resident:
// the counters (wave passes, live lane-passes, the largest pass count of a wave) are there to decide that from numbers.
// ARGARCH's fit is GARCH's on the AR(1) residuals: launch_ar_fit (k_ar_fit<1, 1>, the kernel behind
// arima_fit_batch(1, 0, 0, intercept)) leaves (c, phi) and a status per series in an N x 2 workspace, and
// k_model_fit<ArGarch> forms each residual from the raw row inside the pass (Model::A auxiliary constants per lane), so
// no N x T residual buffer exists. Lanes whose AR stage failed never post a point and report that stage's status.
// k_model_eval<Model>: objective and gradient at caller-given parameters, the same pass routine as the fit's.
// k_model_effects<Model, ADD>, k_ar_effects<ADD>, k_garch_sample<AR>: one streaming pass (md_stream, RowTile<32>::map), N x T
// in, N x T out, independent strides.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sparkts_arima.h"
#include "arima_launch.hpp"
#include "model_pass.hpp"
#include "row_tile.hpp"

namespace sts {

using namespace sts::small;

using MdTile = RowTile<32>;
constexpr int kMdWave = MdTile::kWave;

// The joint pass of one round: f and gradient g at each live lane's point x; rows outside live_mask are not read
template <class Model>
__device__ __forceinline__ void md_wave_pass(MdTile::Lds &tile, const double *rows, int64_t ld, int64_t row0, int T,
                                             int lane, unsigned long long live_mask, bool live, const double *x,
                                             const double *aux, double *f, double *g) {
    typename Model::Pass ps;
    ps.begin(x, aux);
    MdTile::read(tile, rows, ld, row0, T, lane, live_mask, [&](int cb, int n) {
        if (live) {
#pragma unroll 1
            for (int t = cb; t < cb + n; ++t) ps.step(t, tile[lane][t - cb]);
        }
    });
    ps.end(T, f, g);
}

// ctl: [0] wave passes, [1] live lane-passes, [2] the largest pass count of a wave (nullable)
// aux (N x Model::A) / aux_status (N): the per-series constants of the pass and the status of the stage that made them
// (Model::A > 0 only); coef_out is N x Model::NP, the constants first
template <class Model>
__global__ __launch_bounds__(kMdWave) void k_model_fit(const double *__restrict__ rows, int64_t ld, int64_t N, int T,
                                                       const double *__restrict__ aux_all,
                                                       const int32_t *__restrict__ aux_status,
                                                       double *__restrict__ coef_out, double *__restrict__ obj_out,
                                                       int32_t *__restrict__ status_out,
                                                       int32_t *__restrict__ n_eval_out,
                                                       int32_t *__restrict__ n_grad_out, unsigned long long *ctl) {
    constexpr int K = Model::K, A = Model::A, NP = Model::NP;
    __shared__ MdTile::Lds tile;
    const int lane = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kMdWave;
    const int64_t sid = row0 + lane;
    SmallCG<K, Model::kMinimize> m;
    {
        double x0[K];
        Model::initial_guess(x0);
        m.start(x0, 1e-6);                                             // new SimpleValueChecker(1e-6, 1e-6)
    }
    if (sid >= N) m.pc = SmallCG<K, Model::kMinimize>::DONE;          // lanes past N never post a point
    double aux[A > 0 ? A : 1] = {};
    int32_t aux_st = ARIMA_ST_OK;
    if constexpr (A > 0) {
        if (sid < N) {
            aux_st = aux_status[sid];
#pragma unroll
            for (int j = 0; j < A; ++j) aux[j] = aux_all[sid * A + j];
            if (aux_st != ARIMA_ST_OK) m.pc = SmallCG<K, Model::kMinimize>::DONE;      // nor do lanes without constants
        }
    }
    unsigned long long passes = 0, lane_passes = 0;
    for (;;) {
        const bool live = !m.done();
        const unsigned long long live_mask = __ballot(live);
        if (live_mask == 0) break;
        double f, g[K];
        md_wave_pass<Model>(tile, rows, ld, row0, T, lane, live_mask, live, m.xreq(), aux, &f, g);
        if (live) m.advance(f, g);
        ++passes;
        lane_passes += (unsigned long long)__popcll(live_mask);
    }
    if (sid < N) {
        double coef[K], obj;
        m.result(coef, &obj);
        int32_t st = m.status;
        if constexpr (A > 0) {
            // the reference returns no model when either stage throws: every coefficient is NaN then
            if (aux_st != ARIMA_ST_OK) {
                st = aux_st;
                obj = __builtin_nan("");
#pragma unroll
                for (int j = 0; j < K; ++j) coef[j] = __builtin_nan("");
            }
#pragma unroll
            for (int j = 0; j < A; ++j) coef_out[sid * NP + j] = st == ARIMA_ST_OK ? aux[j] : __builtin_nan("");
        }
#pragma unroll
        for (int j = 0; j < K; ++j) coef_out[sid * NP + A + j] = coef[j];
        obj_out[sid] = obj;
        status_out[sid] = st;
        if (n_eval_out) n_eval_out[sid] = m.n_eval;
        if (n_grad_out) n_grad_out[sid] = m.n_grad;
    }
    if (ctl && lane == 0) {
        atomicAdd(&ctl[0], passes);
        atomicAdd(&ctl[1], lane_passes);
        atomicMax(&ctl[2], passes);
    }
}

template <class Model>
__global__ __launch_bounds__(kMdWave) void k_model_eval(const double *__restrict__ rows, int64_t ld, int64_t N, int T,
                                                        const double *__restrict__ params, double *__restrict__ f_out,
                                                        double *__restrict__ g_out) {
    constexpr int K = Model::K;
    __shared__ MdTile::Lds tile;
    const int lane = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kMdWave;
    const int64_t sid = row0 + lane;
    const bool live = sid < N;
    double x[K];
#pragma unroll
    for (int j = 0; j < K; ++j) x[j] = live ? params[sid * K + j] : 0.0;
    double f, g[K];
    md_wave_pass<Model>(tile, rows, ld, row0, T, lane, __ballot(live), live, x, nullptr, &f, g);
    if (live) {
        if (f_out) f_out[sid] = f;
        if (g_out) {
#pragma unroll
            for (int j = 0; j < K; ++j) g_out[sid * K + j] = g[j];
        }
    }
}

// One streaming pass of a wave's rows through fx.step (the entry points refuse any overlap of in_all and out_all)
template <class Fx>
__device__ __forceinline__ void md_stream(MdTile::Lds &tile, Fx &fx, const double *in_all, int64_t ld_in,
                                          double *out_all, int64_t ld_out, int64_t row0, int64_t N, int T, int lane,
                                          bool live) {
    const unsigned long long mask = MdTile::rows_below(row0, N);
    MdTile::map(tile, in_all, ld_in, out_all, ld_out, row0, N, T, lane, mask, [&](int cb, int n) {
        if (live) {
#pragma unroll 1
            for (int t = cb; t < cb + n; ++t) tile[lane][t - cb] = fx.step(t, tile[lane][t - cb]);
        }
    });
}

// params: N x Model::NP (the pass's constants, then the optimizer's parameters)
template <class Model, bool ADD>
__global__ __launch_bounds__(kMdWave) void k_model_effects(const double *__restrict__ in_all, int64_t ld_in,
                                                           const double *__restrict__ params,
                                                           double *__restrict__ out_all, int64_t ld_out, int64_t N,
                                                           int T) {
    constexpr int NP = Model::NP;
    __shared__ MdTile::Lds tile;
    const int lane = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kMdWave;
    const int64_t sid = row0 + lane;
    const bool live = sid < N;
    double x[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) x[j] = live ? params[sid * NP + j] : 0.0;
    typename Model::template Fx<ADD> fx;
    fx.begin(x);
    md_stream(tile, fx, in_all, ld_in, out_all, ld_out, row0, N, T, lane, live);
}

// GARCHModel.sample (AR == false, params N x 3) / ARGARCHModel.sample (AR == true, params N x 5): z in, series out
template <bool AR>
__global__ __launch_bounds__(kMdWave) void k_garch_sample(const double *__restrict__ z_all, int64_t ld_in,
                                                          const double *__restrict__ params,
                                                          double *__restrict__ out_all, int64_t ld_out, int64_t N,
                                                          int T) {
    constexpr int NP = GarchSample<AR>::NP;
    __shared__ MdTile::Lds tile;
    const int lane = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kMdWave;
    const int64_t sid = row0 + lane;
    const bool live = sid < N;
    double x[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) x[j] = live ? params[sid * NP + j] : 0.0;
    GarchSample<AR> fx;
    fx.begin(x);
    md_stream(tile, fx, z_all, ld_in, out_all, ld_out, row0, N, T, lane, live);
}

// ARModel's pair at a runtime order 1 <= p <= kArMaxP; coef N x (1 + p) = (c, phi_1 .. phi_p). Each lane's
// coefficients and its ring of p look-back values live in LDS rows of odd stride (runtime-indexed, so not registers;
// 64 lanes reading the same column of their own rows spread over the banks)
constexpr int kArLdsStride = kArMaxP + 1;
static_assert(kArMaxP == kGenMaxOrder, "ARModel's pair covers the library's order limit");
template <bool ADD>
__global__ __launch_bounds__(kMdWave) void k_ar_effects(const double *__restrict__ in_all, int64_t ld_in,
                                                        const double *__restrict__ coef_all, int p,
                                                        double *__restrict__ out_all, int64_t ld_out, int64_t N,
                                                        int T) {
    __shared__ MdTile::Lds tile;
    __shared__ double cf[kMdWave][kArLdsStride], hist[kMdWave][kArLdsStride];
    const int lane = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kMdWave;
    const int64_t sid = row0 + lane;
    const bool live = sid < N;
    for (int j = 0; j <= p; ++j) cf[lane][j] = live ? coef_all[sid * (1 + p) + j] : 0.0;
    ArFx<ADD> fx;
    fx.begin(cf[lane], p, hist[lane]);
    md_stream(tile, fx, in_all, ld_in, out_all, ld_out, row0, N, T, lane, live);
}

static inline dim3 md_grid(int64_t N) { return dim3((unsigned)((N + kMdWave - 1) / kMdWave)); }

int launch_model_fit(int model, const double *rows, int64_t ld, int64_t N, int T, double *coef_out, double *obj_out,
                     int32_t *status_out, int32_t *n_eval_out, int32_t *n_grad_out, unsigned long long *ctl,
                     hipStream_t s, const double *aux, const int32_t *aux_status) {
    if (N == 0) return ARIMA_OK;
    if (T < 1 || ld < T) return ARIMA_E_INVALID_ARG;
    if (model == kModelEwma)
        hipLaunchKernelGGL((k_model_fit<Ewma>), md_grid(N), dim3(kMdWave), 0, s, rows, ld, N, T, nullptr, nullptr,
                           coef_out, obj_out, status_out, n_eval_out, n_grad_out, ctl);
    else if (model == kModelGarch)
        hipLaunchKernelGGL((k_model_fit<Garch>), md_grid(N), dim3(kMdWave), 0, s, rows, ld, N, T, nullptr, nullptr,
                           coef_out, obj_out, status_out, n_eval_out, n_grad_out, ctl);
    else if (model == kModelArGarch) {
        if (!aux || !aux_status) return ARIMA_E_INVALID_ARG;
        hipLaunchKernelGGL((k_model_fit<ArGarch>), md_grid(N), dim3(kMdWave), 0, s, rows, ld, N, T, aux, aux_status,
                           coef_out, obj_out, status_out, n_eval_out, n_grad_out, ctl);
    } else
        return ARIMA_E_UNSUPPORTED;
    if (hipGetLastError() != hipSuccess) return ARIMA_E_DEVICE;
    return ARIMA_OK;
}

int launch_model_eval(int model, const double *rows, int64_t ld, int64_t N, int T, const double *params, double *f_out,
                      double *g_out, hipStream_t s) {
    if (N == 0) return ARIMA_OK;
    if (T < 1 || ld < T) return ARIMA_E_INVALID_ARG;
    if (model == kModelEwma)
        hipLaunchKernelGGL((k_model_eval<Ewma>), md_grid(N), dim3(kMdWave), 0, s, rows, ld, N, T, params, f_out, g_out);
    else if (model == kModelGarch)
        hipLaunchKernelGGL((k_model_eval<Garch>), md_grid(N), dim3(kMdWave), 0, s, rows, ld, N, T, params, f_out, g_out);
    else
        return ARIMA_E_UNSUPPORTED;
    if (hipGetLastError() != hipSuccess) return ARIMA_E_DEVICE;
    return ARIMA_OK;
}

template <class Model>
static void launch_model_effects_dir(const double *in, int64_t ld_in, const double *params, double *out, int64_t ld_out,
                                     int64_t N, int T, int add, hipStream_t s) {
    if (add)
        hipLaunchKernelGGL((k_model_effects<Model, true>), md_grid(N), dim3(kMdWave), 0, s, in, ld_in, params, out,
                           ld_out, N, T);
    else
        hipLaunchKernelGGL((k_model_effects<Model, false>), md_grid(N), dim3(kMdWave), 0, s, in, ld_in, params, out,
                           ld_out, N, T);
}

int launch_model_effects(int model, const double *in, int64_t ld_in, const double *params, double *out, int64_t ld_out,
                         int64_t N, int T, int add, hipStream_t s) {
    if (N == 0 || T == 0) return ARIMA_OK;
    if (T < 0 || ld_in < T || ld_out < T) return ARIMA_E_INVALID_ARG;
    if (model == kModelEwma) launch_model_effects_dir<Ewma>(in, ld_in, params, out, ld_out, N, T, add, s);
    else if (model == kModelGarch) launch_model_effects_dir<Garch>(in, ld_in, params, out, ld_out, N, T, add, s);
    else if (model == kModelArGarch) launch_model_effects_dir<ArGarch>(in, ld_in, params, out, ld_out, N, T, add, s);
    else return ARIMA_E_UNSUPPORTED;
    if (hipGetLastError() != hipSuccess) return ARIMA_E_DEVICE;
    return ARIMA_OK;
}

int launch_ar_effects(const double *in, int64_t ld_in, const double *coef, int p, double *out, int64_t ld_out,
                      int64_t N, int T, int add, hipStream_t s) {
    if (p < 1) return ARIMA_E_INVALID_ARG;
    if (p > kArMaxP) return ARIMA_E_UNSUPPORTED;
    if (N == 0 || T == 0) return ARIMA_OK;
    if (T < 0 || ld_in < T || ld_out < T) return ARIMA_E_INVALID_ARG;
    if (add)
        hipLaunchKernelGGL((k_ar_effects<true>), md_grid(N), dim3(kMdWave), 0, s, in, ld_in, coef, p, out, ld_out, N, T);
    else
        hipLaunchKernelGGL((k_ar_effects<false>), md_grid(N), dim3(kMdWave), 0, s, in, ld_in, coef, p, out, ld_out, N, T);
    if (hipGetLastError() != hipSuccess) return ARIMA_E_DEVICE;
    return ARIMA_OK;
}

int launch_garch_sample(int model, const double *z, int64_t ld_in, const double *params, double *out, int64_t ld_out,
                        int64_t N, int T, hipStream_t s) {
    if (N == 0 || T == 0) return ARIMA_OK;
    if (T < 0 || ld_in < T || ld_out < T) return ARIMA_E_INVALID_ARG;
    if (model == kModelGarch)
        hipLaunchKernelGGL((k_garch_sample<false>), md_grid(N), dim3(kMdWave), 0, s, z, ld_in, params, out, ld_out, N, T);
    else if (model == kModelArGarch)
        hipLaunchKernelGGL((k_garch_sample<true>), md_grid(N), dim3(kMdWave), 0, s, z, ld_in, params, out, ld_out, N, T);
    else return ARIMA_E_UNSUPPORTED;
    if (hipGetLastError() != hipSuccess) return ARIMA_E_DEVICE;
    return ARIMA_OK;
}

}  // namespace sts
