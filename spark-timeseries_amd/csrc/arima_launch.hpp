// arima_launch.hpp — host-side launchers of the HIP kernels (internal; the public ABI is include/sparkts_arima.h)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sts {

int launch_difference(const double *in, int64_t ld_in, double *out, int64_t ld_out, int64_t N, int T, int d,
                      int drop, hipStream_t s);
int launch_search_init(double *best_aic, int32_t *order, double *coef, int64_t N, hipStream_t s);
constexpr int kSearchMaxLanes = 32;
struct SearchBests {               // the order search's per-lane best candidates (by value into k_search_merge)
    const double *aic[kSearchMaxLanes];
    const int32_t *order[kSearchMaxLanes];
    const double *coef[kSearchMaxLanes];
};
int launch_search_merge(const SearchBests &b, int lanes, int64_t N, double *best_aic, int32_t *order, double *coef,
                        hipStream_t s);
int launch_search_select(const double *cand_coef, const double *cand_ll, const int32_t *cand_status,
                         const uint8_t *cand_flags, int64_t N, int p, int d, int q, int I,
                         const unsigned long long *fit_ctl, double *best_aic, int32_t *order, double *coef,
                         hipStream_t s);
int launch_forecast(const double *ts, int64_t ld_in, const double *coef, int k, double *out, int64_t ld_out,
                    int64_t N, int T, int p, int d, int q, int I, int n_future, hipStream_t s);
int launch_inverse_difference(const double *in, int64_t ld_in, double *out, int64_t ld_out, int64_t N, int T,
                              int d, hipStream_t s);
// ARIMAModel.removeTimeDependentEffects (add == 0) / addTimeDependentEffects (add == 1), p, q <= 5, d <= 8
// (arima_effects.hip); out may be exactly in (same stride)
int launch_effects(const double *in, int64_t ld_in, const double *coef, int k, double *out, int64_t ld_out, int64_t N,
                   int T, int p, int d, int q, int I, int add, hipStream_t s);
// autocorr lags 1 .. max_lag, dwtest and lbtest (statistic, p-value) of every row (arima_diag.hip); every output is
// optional. Lags are served kDgW at a time, a pass pair over the rows per group; with only dw_out, max_lag is ignored
constexpr int kDgW = 8;
int launch_diag(const double *rows, int64_t ld, int64_t N, int T, int max_lag, double *acf_out, double *dw_out,
                double *lb_stat_out, double *lb_pvalue_out, hipStream_t s);
// ---- the small models: EWMA, GARCH(1,1) and ARGARCH (arima_models.hip; cg_small.hpp, model_pass.hpp) ----
// params / coef_out hold NP doubles per series: EWMA (smoothing), GARCH (omega, alpha, beta), ARGARCH (c, phi, omega,
// alpha, beta)
constexpr int kModelEwma = 0, kModelGarch = 1, kModelArGarch = 2;
inline int model_num_params(int model) { return model == kModelEwma ? 1 : model == kModelGarch ? 3 : 5; }
constexpr int kModelCtlWords = 3;  // k_model_fit's counters: wave passes, live lane-passes, the largest pass count of a wave
// EWMA.fitModel / GARCH.fitModel of every row (T >= 1); n_eval_out, n_grad_out and ctl are optional.
// kModelArGarch: the GARCH stage of ARGARCH.fitModel on the raw rows; aux (N x 2) = the AR stage's (c, phi) and
// aux_status (N) its status (launch_ar_fit(p = 1, I = 1)'s coef and status), both required
int launch_model_fit(int model, const double *rows, int64_t ld, int64_t N, int T, double *coef_out, double *obj_out,
                     int32_t *status_out, int32_t *n_eval_out, int32_t *n_grad_out, unsigned long long *ctl,
                     hipStream_t s, const double *aux = nullptr, const int32_t *aux_status = nullptr);
// objective (f_out N) and gradient (g_out N x K, the reference's returned order) at params; either output optional
int launch_model_eval(int model, const double *rows, int64_t ld, int64_t N, int T, const double *params, double *f_out,
                      double *g_out, hipStream_t s);
// removeTimeDependentEffects (add == 0) / addTimeDependentEffects (add == 1); out may not overlap in
int launch_model_effects(int model, const double *in, int64_t ld_in, const double *params, double *out, int64_t ld_out,
                         int64_t N, int T, int add, hipStream_t s);
// ARModel's pair at order 1 <= p <= kGenMaxOrder; coef N x (1 + p) = (c, phi_1 .. phi_p); out may not overlap in
int launch_ar_effects(const double *in, int64_t ld_in, const double *coef, int p, double *out, int64_t ld_out,
                      int64_t N, int T, int add, hipStream_t s);
// GARCHModel.sample (kModelGarch) / ARGARCHModel.sample (kModelArGarch) from the caller's standard normals z
int launch_garch_sample(int model, const double *z, int64_t ld_in, const double *params, double *out, int64_t ld_out,
                        int64_t N, int T, hipStream_t s);
// ---- regressions over a design matrix (arima_regress.hip): AutoregressionX, bgtest, bptest ----
// commons' OLSMultipleLinearRegression over a design that is not made only of a series' own lags. A design has R rows
// and C columns (the ones column included); every column is a window of one source row: value(r) = source[off + r].
constexpr int kRgMaxCols = 64;     // C of k_regress_qr
constexpr int kRgArx = 0, kRgBg = 1, kRgBp = 2, kRgCo = 3;
// RgCol::src: literal 1.0, the per-series row; j >= 0: regressor column j
constexpr int kRgOnes = -2, kRgSelf = -1;
struct RgCol {
    int src, off;
    bool sq;                                       // the value squared (bptest's response)
};
// kind kRgArx: AutoregressionX.fitModel(y, x, lag_a = yMaxLag, lag_b = xMaxLag, orig = includeOriginalX, icpt =
// !noIntercept); kRgBg: bgtest(residuals, factors, lag_a = maxLag); kRgBp: bptest(residuals, factors); kRgCo: the
// pristine copy of RegressionARIMA.fitCochraneOrcutt(y, x), bptest's rows with the response not squared and no ones
// column (icpt = 0). T values per row, k regressor columns
struct RgDesign {
    int kind, T, k, lag_a, lag_b, orig, icpt;
    __host__ __device__ int max_lag() const {
        return kind == kRgBp ? 0 : kind == kRgBg ? lag_a : (lag_a > lag_b ? lag_a : lag_b);
    }
    __host__ __device__ int rows() const { return T - max_lag(); }
    // predictors without the ones column (int64: the entry points check it before anything narrows)
    __host__ __device__ int64_t num_pred() const {
        if (kind == kRgArx) return (int64_t)lag_a + (int64_t)k * lag_b + (orig ? k : 0);
        return (int64_t)k + (kind == kRgBg ? lag_a : 0);
    }
    __host__ __device__ int cols() const { return (int)num_pred() + (icpt ? 1 : 0); }
    // column c of the design in the reference's order; c == cols() is the response
    __host__ __device__ RgCol col(int c) const {
        const int m = max_lag();
        if (c == cols()) return {kRgSelf, m, kind == kRgBp};
        if (icpt && c == 0) return {kRgOnes, 0, false};
        c -= icpt ? 1 : 0;
        if (kind == kRgArx) {                      // y(t-1) .. y(t-a), per column x_c(t-1) .. x_c(t-b), then x_0(t) ..
            if (c < lag_a) return {kRgSelf, m - (c + 1), false};
            c -= lag_a;
            if (c < k * lag_b) return {c / lag_b, m - (c % lag_b + 1), false};
            return {c - k * lag_b, m, false};
        }
        if (c < k) return {c, m, false};           // factors(t, .), then bgtest's u(t-1) .. u(t-maxLag)
        return {kRgSelf, m - (c - k + 1), false};
    }
};
// y: the per-series rows (series or residuals), N x T with row stride ld; x: per series k rows of T values (the
// column-major DenseMatrix(T, k)), series stride xs elements, 0 = one matrix shared by every series
struct RgSrc {
    const double *y;
    int64_t ld;
    const double *x;
    int64_t xs;
    RgSrc at(int64_t f) const { return {y + f * ld, ld, x ? x + f * xs : nullptr, xs}; }
};
// doubles of the workspace of n series: whole blocks of 64 series, element (series 64 b + lane, column c, row r) at
// ws[((b (C + 1) + c) R + r) 64 + lane], column C the response
inline int64_t rg_ws_doubles(int64_t n, int R, int C) { return (n + 63) / 64 * (int64_t)(C + 1) * R * 64; }
// the launchers below need rows() >= 1 and 1 <= cols() <= kRgMaxCols (the entry points report every other shape)
int launch_regress_assemble(const RgDesign &d, const RgSrc &src, int64_t N, double *ws, hipStream_t s);
// commons' QR in place on the assembled workspace, then Solver.solve on the response column: beta (C values) to
// beta_out[i * ldb + boff ..] and, with c_zero, 0.0 to beta_out[i * ldb]; a singular series: status SINGULAR, NaNs
int launch_regress_qr(double *ws, int64_t N, int R, int C, double *beta_out, int ldb, int boff, int c_zero,
                      int32_t *status_out, hipStream_t s);
// calculateRSquared on a freshly assembled workspace: stat = nobs * R^2 and its chi-squared(df) upper tail; NaNs where
// status is not OK. beta N x C
int launch_regress_r2(const double *ws, const double *beta, const int32_t *status, int64_t N, int R, int C, int nobs,
                      int df, double *stat_out, double *pvalue_out, hipStream_t s);
// ARXModel.predict straight from the sources: coef N x (1 + K) = (c, coefficients), out N x rows() (row stride ld_out)
int launch_arx_predict(const RgDesign &d, const RgSrc &src, const double *coef, double *out, int64_t ld_out, int64_t N,
                       hipStream_t s);
// RegressionARIMA.fitCochraneOrcutt, the whole iteration of every series in one launch. ps: the kRgCo design of the n
// series as launch_regress_assemble wrote it (rg_ws_doubles(n, T, k) doubles: x_0 .. x_{k-1}, then y), read only; wk:
// rg_ws_doubles(n, T, k + 1) doubles of working design, rebuilt and destroyed once per QR. coef_out N x (1 + k)
// (intercept first), rho_out N, n_iter_out N (nullable): the iterations run, also for a failed series; status_out N.
// Needs 1 <= k, k + 1 <= T and k + 1 <= kRgMaxCols (the entry points report every other shape)
int launch_cochrane_orcutt(const double *ps, double *wk, int64_t N, int T, int k, int max_iter, double *coef_out,
                           double *rho_out, int32_t *n_iter_out, int32_t *status_out, hipStream_t s);
// a shape the reference refuses for every series alike: status to status_out, NaN to the n0 / n1 doubles per series
// of out0 / out1 (null: none)
int launch_regress_refuse(int64_t N, int32_t status, int32_t *status_out, double *out0, int n0, double *out1, int n1,
                          hipStream_t s);
// The fit kernel's counter words (ctl) and express-ring ready words are initialised by the kernel that runs before it
// on the same stream (k_hr_init, else k_fit_prep): ctl[] = 0 except ctl[15] = ~0 and the option words 19, 44-47;
// xready[0 .. xready_words) = 0. ctl == nullptr / xready_words == 0: nothing to prepare.
// Words 0-47 are the block fit_stats.hpp sums and the order search accumulates word by word; kFitCtlSkippedG follows it.
constexpr int kFitCtlSkippedG = 48;          // gradient evaluations the optimizer counted without a pass (CGLane SKIPG)
constexpr int kFitCtlWords = 49;
struct FitPrep {
    unsigned long long *ctl = nullptr;
    unsigned *xready = nullptr;
    int64_t xready_words = 0;
    unsigned long long v19 = 0, v44 = 0, v45 = 0, v46 = 0, v47 = 0;
};
int launch_fit_prep(const FitPrep &prep, hipStream_t s);
// hr_grid > 0: that many single-wave workgroups stride over the series (bounds the rows in flight, so the 2(C_A + C_B)
// passes over a row can hit the Infinity Cache); 0: one lane per series in 256-lane workgroups.
// dd (here and in the fit launchers): 1 = y holds the RAW rows of a d = 1 fit and every pass differences them on the
// fly (arima_device.hpp stream_row); 0 = y holds the differenced rows.
int launch_hr_init(const double *y, int64_t ld, int n, int64_t N, int p, int q, int I, double *init_out,
                   int32_t *status_out, hipStream_t s, int hr_grid = 0, int dd = 0, const FitPrep &prep = FitPrep{});
// The per-series outputs of a fit: coef is N x k, the others N; n_eval, n_grad and flags are optional (null).
// at(first, k): the bundle `first` rows further on (coefficient rows of k doubles); null members stay null
struct FitOut {
    double *coef, *ll; int32_t *status, *n_eval, *n_grad; uint8_t *flags;
    FitOut at(int64_t f, int k) const {
        return {coef ? coef + f * k : nullptr, ll ? ll + f : nullptr,         status ? status + f : nullptr,
                n_eval ? n_eval + f : nullptr, n_grad ? n_grad + f : nullptr, flags ? flags + f : nullptr};
    }
};
int launch_ar_fit(const double *y, int64_t ld, int n, int64_t N, int p, int I, const FitOut &out, hipStream_t s,
                  int dd = 0);
int launch_cg_fit(const double *y, int64_t ld, int n, int64_t N, int p, int q, int I, int smear, const double *init,
                  const int32_t *init_status, const FitOut &out, unsigned long long *ctl, int grid_blocks,
                  int express_blocks, unsigned char *xq, unsigned *xready, int join_express, hipStream_t s, int dd = 0);
constexpr int kExpressRingEntries = 32768;      // k_cg_fit's express hand-offs per launch (entries never reused)
constexpr int kExpressRingBytes = kExpressRingEntries * 512;   // x kExpressEntryBytes
constexpr int kExpressReadyBytes = kExpressRingEntries * 4;
int launch_css_loglik(const double *y, int64_t ld, int n, int64_t N, int p, int q, int I, const double *coef,
                      double *ll_out, hipStream_t s);
int launch_css_grad(const double *y, int64_t ld, int n, int64_t N, int p, int q, int I, int smear,
                    const double *coef, double *g_out, hipStream_t s);
int launch_model_flags(const double *coef, int64_t N, int p, int q, int I, uint8_t *flags_out, hipStream_t s);
// base_host: I + p + q host doubles (passed to the kernel by value)
int launch_sample(double *out, int64_t ld, int64_t N, int T, int p, int d, int q, int I, const double *base_host,
                  double jitter, uint64_t seed, int64_t first, hipStream_t s);
int cg_fit_series_per_block(int p, int q, int I);   // optimizer slots of one fit workgroup
// k_cg_fit workgroups are single waves (4 per CU, one per SIMD, each with a quarter of the LDS): a wave that has
// finished its series leaves the CU at once, so the next fit's waves take its SIMD and LDS share while the other
// waves of the CU still run their slowest series (pipelined fits)
constexpr int kFitBlockWaves = 1;            // waves per k_cg_fit workgroup
constexpr int kFitWavesPerCU = 4;            // resident k_cg_fit waves per CU (one per SIMD)
constexpr int kFitBlocksPerCU = kFitWavesPerCU / kFitBlockWaves;

constexpr int kMergeLiveDefault = 16;        // k_cg_fit's drain merge threshold (option "merge_live"; 0 = off)

// ---- ARIMA.autoFit (arima_autofit.hip) ----
// candidate (p, q, intercept) orders the stepwise walk can meet: p <= max(max_p, 2), q <= 2 (combo (p * 3 + q) * 2 + I;
// max_p <= kAfMaxP: its css-bobyqa retries have at most 11 parameters, the dimensions arima_bobyqa.hip compiles)
constexpr int kAfMaxP = 8;
constexpr int kAfCombosMax = (kAfMaxP + 1) * 6;
inline int af_combos(int max_p) { return ((max_p > 2 ? max_p : 2) + 1) * 6; }
constexpr int kAfMaxCand = 4;      // distinct candidates of one round of one series
struct AfSeries {                  // one series' walk state (findBestARMAModel's locals, ARIMA.scala:321-375)
    double best_aic;               // curBestAIC
    unsigned long long seen;       // pastParams, one bit per (p, q, intercept)
    int32_t dsel;                  // d chosen by the KPSS search (-1: none)
    int32_t status;                // ARIMA_ST_*
    int32_t best;                  // packed p | q << 4 | I << 8 of curBestModel, -1 = null
    int32_t n_fits;                // candidate fits run so far
    int32_t ncand;                 // candidates of the current round (0: the walk is over)
    int32_t cand[kAfMaxCand];      // nextParams, packed, deduplicated in first-appearance order
    int32_t slot[kAfMaxCand];      // each candidate's row in its order's list this round
};
int launch_kpss_c(const double *w, int64_t ld, int n, int64_t N, int d, int32_t *dsel, double *stat_out, hipStream_t s);
int kpss_lag_host(int n);
int kpss_lag_max();
int launch_difference_sel(const double *in, int64_t ld_in, double *out, int64_t ld_out, int64_t N, int T,
                          const int32_t *dsel, int d, hipStream_t s);
int launch_af_init(int64_t N, const int32_t *dsel, AfSeries *st, int32_t kpss_status, hipStream_t s);
int launch_af_plan(int64_t N, AfSeries *st, unsigned *counts, int32_t *lists, hipStream_t s);
int launch_gather_rows(const double *in, int64_t ld, const int32_t *list, int64_t count, int T, double *out,
                       hipStream_t s);
int launch_af_update(int64_t N, AfSeries *st, const int64_t *off, const double *res_coef, const double *res_ll,
                     const int32_t *res_status, const uint8_t *res_flags, double *best_coef, int max_p, int max_q,
                     hipStream_t s);
int launch_af_finish(int64_t N, const AfSeries *st, const double *best_coef, int32_t *order_out, double *coef_out,
                     double *aic_out, int32_t *status_out, int32_t *n_fits_out, hipStream_t s);

// css-bobyqa (arima_bobyqa.hip): one lane per series after the initial parameters; refit_status (optional): only the
// series whose css-cgd status there is an optimizer exception (autoFit's fitTryBothStrategies) are refitted in place
int launch_bobyqa_fit(const double *y, int64_t ld, int n, int64_t N, int p, int q, int I, const double *init,
                      const int32_t *init_status, const int32_t *refit_status, const FitOut &out, bool wave,
                      hipStream_t s);

// autoFit: the css-bobyqa retries of a whole round (every order's rows whose css-cgd fit threw in the optimizer), one
// launch; rows = the differenced series (ld), lists / off = the round's per-order lists and row offsets, init /
// init_status = each row's Hannan-Rissanen init (k-strided from off[cb] * 11) and status; list / count: workspace
// (the list, bucketed by dimension k = p + q + intercept -- bucket k at list[k * stride ..], counts[k] rows -- then
// one kernel per dimension present, each on its own stream; ncombos orders in the round's layout, coefficient rows
// kc-strided from off[cb] * kc)
constexpr int kBqRefitBuckets = 12;
int launch_bobyqa_refit_list(const int64_t *off, int ncombos, int64_t total, const int32_t *status, int32_t *list,
                             int64_t stride, unsigned *counts, hipStream_t s);
int launch_bobyqa_refit_dim(int k, const double *rows_, int64_t ld, int n, const int32_t *lists, int64_t N,
                            const int64_t *off, int ncombos, int kc, const int32_t *list, const unsigned *counts,
                            int64_t rows, const double *init, const int32_t *init_status, const FitOut &out, bool wave,
                            hipStream_t s);

int hr_shape_status_host(int n, int p, int q, int I);
int ar_shape_status_host(int n, int p, int I);

// ---- the runtime-order path (arima_generic.hip): p or q above the compiled orders (5), up to kGenMaxOrder ----
constexpr int kFastMaxOrder = 5;   // orders the compile-time kernels cover
constexpr int kGenMaxOrder = 20;   // p, q <= 20
constexpr int kGenMaxK = 2 * kGenMaxOrder + 1;
inline bool gen_order(int p, int q) { return p > kFastMaxOrder || q > kFastMaxOrder; }
// Fused differencing pays where the fused Householder init keeps its registers (k_hr_init<P, Q, I, true>): C2's
// (2,1,2)+c gains 7 % from it, C4's (5,1,5)+c loses 6-16 % (profiles/r06/d_ab, p_c4fuse, q_fuse); the compiled orders
// with p + q <= 6 fuse, the others take the k_difference copy. The runtime-order kernels always fuse.
inline bool fuse_pays(int p, int q) { return gen_order(p, q) || p + q <= 6; }
bool gen_orders_ok(int p, int q);
int launch_gen_hr_init(const double *y, int64_t ld, int n, int64_t N, int p, int q, int I, double *init_out,
                       int32_t *status_out, int dd, const FitPrep &prep, hipStream_t s);
int launch_gen_ar_fit(const double *y, int64_t ld, int n, int64_t N, int p, int I, const FitOut &out, int dd,
                      hipStream_t s);
int launch_gen_fit(const double *y, int64_t ld, int n, int64_t N, int p, int q, int I, int smear, const double *init,
                   const int32_t *init_status, const FitOut &out, unsigned long long *ctl, int dd, hipStream_t s);
int launch_gen_css_loglik(const double *y, int64_t ld, int n, int64_t N, int p, int q, int I, const double *coef,
                          double *ll_out, hipStream_t s);
int launch_gen_css_grad(const double *y, int64_t ld, int n, int64_t N, int p, int q, int I, int smear,
                        const double *coef, double *g_out, hipStream_t s);
int launch_gen_model_flags(const double *coef, int64_t N, int p, int q, int I, uint8_t *flags_out, hipStream_t s);
int64_t gen_forecast_ws_doubles(int T, int p, int d, int q, int n_future);
int launch_gen_forecast(const double *ts, int64_t ld_in, const double *coef, int k, double *out, int64_t ld_out,
                        int64_t N, int T, int p, int d, int q, int I, int n_future, double *ws, int64_t ws_stride,
                        hipStream_t s);
// launch_effects at any order the library accepts (p, q <= kGenMaxOrder, d <= 16); no workspace
int launch_gen_effects(const double *in, int64_t ld_in, const double *coef, int k, double *out, int64_t ld_out,
                       int64_t N, int T, int p, int d, int q, int I, int add, hipStream_t s);

// ---- ARIMAX (arima_arimax.hip): K' = 1 + p + q + nX coefficients, nX = k * xregMaxLag + (includeOriginalXreg ? k : 0)
// p, q <= kGenMaxOrder and 1 <= K' <= kGenMaxK
bool arimax_shape_ok(int p, int q, int Kp);
// fitModel's start point: arx N x (1 + p + nX) and its status (launch_regress_qr's), hr N x max(I + p + q, 1) and its
// status (launch_hr_init's) -> init N x K' and the merged status, the ARX status first
int launch_arimax_splice(const double *arx, const int32_t *arx_status, const double *hr, const int32_t *hr_status,
                         int64_t N, int p, int q, int I, int nX, double *init, int32_t *status, hipStream_t s);
// fitWithCSSCGD over all K' coordinates of the differenced rows y (n values, row stride ld); init N x K', init_status
// nullable (a series whose status there is not OK gets it, NaN outputs and no fit); out.flags is not written
int launch_arimax_fit(const double *y, int64_t ld, int n, int64_t N, int p, int q, int I, int Kp, int smear,
                      const double *init, const int32_t *init_status, const FitOut &out, hipStream_t s);
// the streaming kernel (arima_kernels.hip): p, q <= kFastMaxOrder and d <= 8, else ARIMA_E_UNSUPPORTED; no workspace
int launch_arimax_forecast_stream(const double *ts, int64_t ld_in, const double *x, int64_t xs, int kx,
                                  const double *coef, int Kp, double *out, int64_t ld_out, int64_t N, int T, int p,
                                  int d, int q, int I, int L, int orig, int n_future, hipStream_t s);
// every other order: the reference's arrays in a workspace, as launch_gen_forecast
int64_t arimax_forecast_ws_doubles(int T, int p, int d, int q, int n_future);
// ARIMAXModel.forecast: x per series kx columns of n_future values (series stride xs, 0 = shared), coef N x K',
// out N x T; ws: ws_stride >= arimax_forecast_ws_doubles doubles per series. Shapes the reference throws for are
// ARIMA_E_INVALID_ARG
int launch_arimax_forecast(const double *ts, int64_t ld_in, const double *x, int64_t xs, int kx, const double *coef,
                           int Kp, double *out, int64_t ld_out, int64_t N, int T, int p, int d, int q, int I, int L,
                           int orig, int n_future, double *ws, int64_t ws_stride, hipStream_t s);

}  // namespace sts
