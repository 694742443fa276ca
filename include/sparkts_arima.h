/*
 * sparkts_arima.h — C ABI of the MI355X-native batched ARIMA (CSS-CGD) engine.
 *
 * This library is a drop-in for ONE hot path of spark-ts (dhmodi/spark-timeseries, sparkts 0.4.0-SNAPSHOT):
 *
 *     ARIMA.fitModel(p, d, q, ts, includeIntercept, method = "css-cgd", userInitParams)
 *         src/main/scala/com/cloudera/sparkts/models/ARIMA.scala:79-116
 *
 * called once per series inside TimeSeriesRDD.mapSeries (TimeSeriesRDD.scala:249-260). The JVM binding
 * a maintainer adds on the reference side (JNI / Panama) is shown in INTEGRATION.md; the Python mirror of
 * python/sparkts/models/ARIMA.py lives in spark-timeseries_amd/sparkts_amd/.
 *
 * Conventions
 *   - Plain C types only. Host-buffer entry points take caller-owned host memory; the library never keeps a
 *     pointer after return. `*_device` entry points take device (HBM) pointers and a hipStream_t passed as
 *     `void*` (NULL = the handle's own stream) and are asynchronous w.r.t. the host: they enqueue their work
 *     and return (results are valid once that stream reaches the call's end). Calls on one handle are also
 *     ordered on the device whichever streams they use, because they share the handle's workspaces --
 *     except fit calls under the "fit_pipeline" option (arima_set_option; default 3): consecutive
 *     arima_fit_batch_device calls rotate over P fit contexts and may run concurrently -- unless a call's
 *     buffers overlap an in-flight call's (it reads that call's outputs, writes its inputs, or writes the same
 *     outputs): then it waits for that call, whatever fit_pipeline is set to when it is issued, so results always
 *     equal fit_pipeline 1's. Every non-fit call
 *     still waits for all earlier calls. arima_get_last_stats waits for the last call's device work.
 *     Host-buffer entry points block (arima_fit_batch pipelines its own chunks internally: "host_chunk",
 *     "host_pipeline").
 *   - A batch is N series of equal length T, series-major: element t of series i is series[i*ld + t]
 *     (ld == T for the host-buffer entry points). One call = one Spark partition bucketed by length.
 *   - Coefficient layout per series is the reference's: [c?, phi_1..phi_p, theta_1..theta_q]
 *     (ARIMA.scala:74-77, 406); k = arima_num_params(p, q, include_intercept).
 *   - Return value: ARIMA_OK or a negative ARIMA_E_* (API misuse / device failure only). Per-series
 *     outcomes are reported in status_out (ARIMA_ST_*), one code per exception the reference can throw on
 *     this path; a failed series never aborts the batch and its coefficients are NaN.
 */
#ifndef SPARKTS_ARIMA_H
#define SPARKTS_ARIMA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- call-level return codes ---------------------------------------------------------------------- */
#define ARIMA_OK              0
#define ARIMA_E_INVALID_ARG  (-1)
#define ARIMA_E_UNSUPPORTED  (-2)
#define ARIMA_E_DEVICE       (-3)
#define ARIMA_E_OOM          (-4)

/* ---- per-series status: one code per reference outcome ----------------- */
#define ARIMA_ST_OK                  0  /* fit returned normally                                             */
#define ARIMA_ST_MAX_EVAL            1  /* commons TooManyEvaluationsException, MaxEval(10000) ARIMA.scala:196 */
#define ARIMA_ST_BRACKET_MAX_EVAL    2  /* commons BracketFinder's own 500-evaluation cap                    */
#define ARIMA_ST_MAX_ITER            3  /* commons TooManyIterationsException, MaxIter(10000) ARIMA.scala:195 */
#define ARIMA_ST_SINGULAR            4  /* commons SingularMatrixException (QR rDiag == 0), ARIMA.scala:240   */
#define ARIMA_ST_NOT_ENOUGH_DATA     5  /* MathIllegalArgumentException: rows < predictors + 1               */
#define ARIMA_ST_NO_DATA             6  /* NoDataException: zero rows, or zero columns without intercept     */
#define ARIMA_ST_BAD_INTERVAL        7  /* NumberIsTooLarge / OutOfRange from SearchInterval (line search)   */
#define ARIMA_ST_ZERO_PARAMS         8  /* k == 0 parameters (ArithmeticException / index error)             */
#define ARIMA_ST_UNSUPPORTED_METHOD  9  /* UnsupportedOperationException, ARIMA.scala:108 (unknown method)    */
#define ARIMA_ST_SERIES_TOO_SHORT   10  /* negative lag-matrix size (NegativeArraySize / IndexOutOfBounds)    */
/* ARIMA.autoFit outcomes (ARIMA.scala:280-375), arima_autofit_batch* only */
#define ARIMA_ST_NOT_STATIONARY     11  /* no d <= max_d passes the KPSS test: "stationarity not achieved", :293-296 */
#define ARIMA_ST_NO_MODEL           12  /* no candidate qualified: curBestModel stays null (NullPointerException)  */
/* 13 and 15 are retired: they reported BOBYQA's RESCUE branch before it was restated (round 6); never returned */
/* css-bobyqa outcomes (ARIMA.fitWithCSSBOBYQA, ARIMA.scala:130-160) */
#define ARIMA_ST_TOO_FEW_PARAMS     14  /* BOBYQAOptimizer needs >= 2 parameters (NumberIsTooSmallException)    */

/* ---- fit methods (ARIMA.scala:105-109) -------------------------------------------------------------- */
#define ARIMA_METHOD_CSS_CGD     0
#define ARIMA_METHOD_CSS_BOBYQA  1      /* commons BOBYQAOptimizer as ARIMA.fitWithCSSBOBYQA configures it (ARIMA.scala:130-160) */

/* ---- stationarity / invertibility flags (ARIMAModel.isStationary / isInvertible, ARIMA.scala:777-815) - */
#define ARIMA_FLAG_STATIONARY  1u
#define ARIMA_FLAG_INVERTIBLE  2u

typedef struct arima_handle arima_handle;

/* Aggregate counters of the last fit call on a handle (for roofline accounting). */
typedef struct arima_fit_stats {
    int64_t n_series;
    int64_t f_passes;        /* objective (CSS) passes actually executed over a series            */
    int64_t g_passes;        /* gradient passes actually executed over a series (each also yields CSS) */
    int64_t hr_passes;       /* Hannan-Rissanen streaming-QR passes executed                       */
    int64_t n_eval;          /* objective evaluations as counted by the reference (incl. memoised)  */
    int64_t n_grad;          /* gradient evaluations as counted by the reference                    */
                             /* (both from the css-cgd kernels' counters; after arima_fit_batch also for css-bobyqa and
                              * the AR-only shortcut, summed from the per-series results; 0 for those after a *_device fit) */
    double  flops;           /* algorithmic flops of all passes executed (SURVEY.md 8(d) formula)   */
    double  ms_difference;   /* device time of each kernel of the last call (HIP events, ms)        */
    double  ms_hr_init;
    double  ms_cg_fit;
    double  ms_total;
    int64_t wave_f_passes;   /* wave-level objective-only passes of the fit kernel                   */
    int64_t wave_g_passes;   /* wave-level passes that included the gradient recursion               */
    int64_t grid_blocks;     /* workgroups of the persistent fit kernel                               */
    int64_t spec_hits;       /* objective evaluations answered by a speculative line-search point     */
    int64_t wave_multi_passes; /* wave-level objective passes that carried speculative points          */
    int64_t spec_chains;     /* objective chains evaluated by lane F passes (primary + speculative)    */
    int64_t express_blocks;  /* CUs of express workgroups in the fit kernel (long-running series) */
    int64_t express_series;  /* series finished on the express path                                    */
    int64_t express_f_passes; /* objective / gradient passes run on the express path                    */
    int64_t express_g_passes;
    int64_t fault;           /* != 0: the fit kernel's hand-off watchdog fired (1 = stall, 2 = lost request, 3 = merge stall);
                                the call also returns ARIMA_E_DEVICE from arima_synchronize / blocking entry points */
    int64_t fault_info[5];   /* the kernel's record of the first fault (ticket, fills, bulk waves done, ...)      */
    int64_t diag[6];         /* diagnostics of builds with -DSTS_TIMING; else 0                       */
    int64_t ride_passes;     /* objective requests served by gradient passes (counted in g_passes)    */
    int64_t series_done;     /* series whose result the fit kernels wrote (== n_series unless a fault dropped some) */
    int64_t express_pit_passes;  /* express objective passes run parallel in time (all lanes on one series)   */
    int64_t express_pit_sweeps;  /* block sweeps of the parallel-in-time passes (objective and gradient)     */
    int64_t express_pit_g_passes;    /* express gradient passes run parallel in time                        */
    int64_t wave_chains;         /* objective chains the bulk objective passes computed (64 x chains per pass) */
    int64_t low_util_passes;     /* bulk wave passes that served fewer than 32 lanes                         */
    int64_t diag_step_cycles;    /* STS_TIMING builds: optimizer-step cycles, and refill cycles (within diag[2]) */
    int64_t diag_refill_cycles;
    int64_t merge_series;        /* series the drain merge moved between bulk waves (option "merge_live")    */
    int64_t merge_waves;         /* bulk waves that handed their last series over and left                   */
    int64_t skipped_g;           /* gradient evaluations counted in n_grad that ran no pass: after a line search whose
                                    result the next iteration's test stops on, nothing reads the gradient. For css-cgd
                                    fits whose points stay finite: g_passes - ride_passes + express_g_passes + skipped_g
                                    == n_grad */
} arima_fit_stats;

/* ---- lifecycle ------------------------------------------------------------------------------------- */
/* One handle per device. Calls on one handle are serialised internally (thread-safe). arima_get_last_stats
 * waits for the device work of the last fit on the handle (the fit calls themselves do not). */
int         arima_create(int device, arima_handle **out);
int         arima_destroy(arima_handle *h);
const char *arima_last_error(const arima_handle *h);
const char *arima_status_name(int status);
int         arima_num_params(int p, int q, int include_intercept);
int         arima_get_last_stats(const arima_handle *h, arima_fit_stats *out);
/* Blocks until the device work of every call issued on the handle so far has finished. */
int         arima_synchronize(arima_handle *h);
/* Orders: p, q <= 5 run the order-specialised kernels, 5 < p, q <= 20 the runtime-order path (arima_generic.hip: the
 * same results, not tuned); p or q > 20 return ARIMA_E_UNSUPPORTED, and so do css-bobyqa fits of more than 11
 * parameters (the dimensions its kernels compile) and autoFit with max_p > 8 (its css-bobyqa retries).
 * Tuning knobs (not part of the reference contract): "smear" (Breeze reading at ARIMA.scala:526, default 1),
 * "fit_pipeline" (fit contexts in rotation for *_device fits, 1..8, default 3), "host_chunk" / "host_pipeline"
 * (series per chunk and contexts of the chunked host path: 131072 / 6 when GPU_MAX_HW_QUEUES >= 8 at arima_create, else
 * 262144 / 3), "host_tail" (1: the host path halves its last chunks, down to 16384 series; a tail chunk never
 * exceeds "host_chunk", so a "host_chunk" below 16384 keeps its own size to the end), "express_blocks",
 * "grid_blocks", "search_lanes" (in-kernel scheduler and order-search concurrency), "hr_grid" (k_hr_init grid:
 * 0 = a lane per series, > 0 = that
 * many single-wave workgroups, -1 = 1024 for pipelined fits else 0), "fit_slice_bytes"
 * (differenced workspace of one slice of a large device fit), "express_ring" (express hand-offs per launch),
 * "row_pad" (doubles added to the stride of the differenced-row workspaces, whole 128-B lines, default 0),
 * "merge_live" (k_cg_fit drain merge: after the batch's work counter ran out, a wave with at most this many live
 * series hands them to waves still running and exits, 0..64, 0 = off; results never depend on it),
 * "search_express_blocks" (express CUs of each concurrent order-search fit, default 0; -1 = as "express_blocks"),
 * "donate_evals" / "donate_evals_drained" (evaluations before a series may move to an express wave, before / after
 * the batch's work counter ran out; 0 = the kernel's 256 / 32), "fuse_diff" (1, default: device fits of d <= 1 read the
 * caller's rows and difference them inside every pass where that pays -- compiled orders with p + q <= 6, every
 * runtime order; 2: at every order; 0: always through a k_difference workspace -- identical results),
 * "autofit_slice" (autoFit series per slice of its workspaces, 0 = from free HBM), "host_copy_threads" (host threads
 * that copy arima_fit_batch's rows into pinned blocks for the upload; default 0 = upload from pageable memory through
 * the HIP runtime's staging), "chain_overhead" (k_cg_fit's objective-pass width model; 0 = the kernel's),
 * "diag_slice_bytes" (residual workspace of one slice of arima_residual_diagnostics_batch*; 0, the default, = 60 % of
 * the free HBM, at least 1 GiB; results never depend on it), "regress_slice_bytes" (design workspace of one slice of
 * the arima_arx_*, arima_bgtest_* and arima_bptest_* calls; 0, the default, = the same rule; results never depend on
 * it). */
int         arima_set_option(arima_handle *h, const char *name, int64_t value);
/* Current value of a tuning knob (the names arima_set_option takes); ARIMA_E_INVALID_ARG for an unknown name. */
int         arima_get_option(const arima_handle *h, const char *name, int64_t *value);

/* ---- ARIMA.fitModel over a batch (ARIMA.scala:79-116) ----------------------------------------------- *
 * series    N x T host, series-major                 user_init  NULL (Hannan-Rissanen, ARIMA.scala:216) or N x k
 * coef_out  N x k                                    css_ll_out N: logLikelihoodCSS at coef_out (ARIMA.scala:417)
 * status_out N (ARIMA_ST_*)                          n_eval_out / n_grad_out: N, nullable (reference counters)
 * flags_out N, nullable (ARIMA_FLAG_*)                                                                     */
int arima_fit_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                    int32_t p, int32_t d, int32_t q, int32_t include_intercept, int32_t method,
                    const double *user_init, double *coef_out, double *css_ll_out, int32_t *status_out,
                    int32_t *n_eval_out, int32_t *n_grad_out, uint8_t *flags_out);

/* Same, device-resident: every pointer is device memory; `ld` is the row stride (elements) of d_series. */
int arima_fit_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T, int64_t ld,
                           int32_t p, int32_t d, int32_t q, int32_t include_intercept, int32_t method,
                           const double *d_user_init, double *d_coef_out, double *d_css_ll_out,
                           int32_t *d_status_out, int32_t *d_n_eval_out, int32_t *d_n_grad_out,
                           uint8_t *d_flags_out, void *stream);

/* ---- building blocks of the path (each mirrors one reference function; host buffers) --------------- */
/* UnivariateTimeSeries.differencesOfOrderD (UnivariateTimeSeries.scala:468-480): size-preserving, N x T out */
int arima_difference_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T, int32_t d,
                           double *out);
/* UnivariateTimeSeries.inverseDifferencesOfOrderD (UnivariateTimeSeries.scala:489-495), N x T out */
int arima_inverse_difference_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                                   int32_t d, double *out);
/* ARIMAModel.logLikelihoodCSS (ARIMA.scala:417-420): differences to order d, drops d, CSS log-likelihood */
int arima_css_loglik_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                           int32_t p, int32_t d, int32_t q, int32_t include_intercept, const double *coef,
                           double *ll_out);
/* ARIMAModel.gradientlogLikelihoodCSSARMA (ARIMA.scala:465-534) on already-differenced series (length n) */
int arima_css_gradient_batch(arima_handle *h, const double *diffed, int64_t n_series, int32_t n,
                             int32_t p, int32_t q, int32_t include_intercept, const double *coef,
                             double *grad_out);
/* ARIMA.hannanRissanenInit (ARIMA.scala:216-242) on already-differenced series (length n), N x k out */
int arima_hannan_rissanen_batch(arima_handle *h, const double *diffed, int64_t n_series, int32_t n,
                                int32_t p, int32_t q, int32_t include_intercept, double *init_out,
                                int32_t *status_out);
/* ARIMAModel.forecast (ARIMA.scala:696-764): N x (T + n_future) out */
int arima_forecast_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                         int32_t p, int32_t d, int32_t q, int32_t include_intercept, const double *coef,
                         int32_t n_future, double *out);
/* Same, device-resident: d_series N x T (row stride ld), d_coef N x k, d_out N x (T + n_future) (row stride ld_out) */
int arima_forecast_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T, int64_t ld,
                                int32_t p, int32_t d, int32_t q, int32_t include_intercept, const double *d_coef,
                                int32_t n_future, double *d_out, int64_t ld_out, void *stream);
/* ---- the TimeSeriesModel pair of ARIMAModel (TimeSeriesModel.scala:23-45), N x T in, N x T out ---------------- *
 * ARIMAModel.removeTimeDependentEffects (ARIMA.scala:629-644): the residuals of each series under its model --
 * differencesOfOrderD(ts, d) (size-preserving, nothing dropped), then iterateARMA with op = - whose errors are its own
 * output. What lbtest / dwtest / bgtest (TimeSeriesStatisticalTests.scala:251-320) take as input.
 * ARIMAModel.addTimeDependentEffects (ARIMA.scala:655-667): each model driven by the caller's innovations (`noise`)
 * -- iterateARMA with op = + on its own output, then inverseDifferencesOfOrderD(_, d); `sample` (:675-678) is this
 * over Gaussian noise.
 * coef N x k. T < d returns ARIMA_E_INVALID_ARG; N == 0 or T == 0 return ARIMA_OK and write nothing. One streaming
 * pass (p, q <= 5 and d <= 8: the tiled kernel; every other accepted order: the runtime-order kernel).
 * `out` may be exactly the input (the reference's sample calls addTimeDependentEffects(vec, vec)): the same pointer
 * and, for the device entry points, the same stride; any other overlap of the two ranges, or of out and coef,
 * returns ARIMA_E_INVALID_ARG. Nothing is written beyond column T of a row.                                        */
int arima_remove_effects_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                               int32_t p, int32_t d, int32_t q, int32_t include_intercept, const double *coef,
                               double *out);
int arima_add_effects_batch(arima_handle *h, const double *noise, int64_t n_series, int32_t T,
                            int32_t p, int32_t d, int32_t q, int32_t include_intercept, const double *coef,
                            double *out);
/* Same, device-resident: d_series / d_noise N x T (row stride ld >= T), d_coef N x k, d_out N x T (row stride
 * ld_out >= T) */
int arima_remove_effects_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T,
                                      int64_t ld, int32_t p, int32_t d, int32_t q, int32_t include_intercept,
                                      const double *d_coef, double *d_out, int64_t ld_out, void *stream);
int arima_add_effects_batch_device(arima_handle *h, const double *d_noise, int64_t n_series, int32_t T,
                                   int64_t ld, int32_t p, int32_t d, int32_t q, int32_t include_intercept,
                                   const double *d_coef, double *d_out, int64_t ld_out, void *stream);
/* ---- residual diagnostics: autocorr, dwtest, lbtest over a batch ---------------------------------------------- *
 * Per row of N x T: UnivariateTimeSeries.autocorr(ts, max_lag) (UnivariateTimeSeries.scala:70-96) into acf_out
 * N x max_lag (lag i at column i - 1), TimeSeriesStatisticalTests.dwtest (TimeSeriesStatisticalTests.scala:251-262)
 * into dw_out N, and lbtest(ts, max_lag) (:298-307) into lb_stat_out N and lb_pvalue_out N. Every output may be NULL.
 * acf, dw and the statistic are the reference's arithmetic in its order (nothing special-cased: a constant row or
 * T - lag == 1 give NaN correlations, NaN and Inf propagate, and the Int product n * (n + 2) of lbtest wraps for
 * T >= 46340, after which the statistic is negative and the p-value 1). The p-value restates commons-math3's
 * chi-squared tail and agrees with it to a tolerance, not to bits (csrc/arima_chisq.hpp); where the library would
 * throw (an infinite statistic) it is NaN.
 * With any of acf_out, lb_stat_out, lb_pvalue_out requested, max_lag must be in [1, T - 1] (the reference's slicing
 * and ChiSquaredDistribution(0) throw otherwise): ARIMA_E_INVALID_ARG. With only dw_out, max_lag is ignored.
 * N == 0 or T == 0 return ARIMA_OK and write nothing. Outputs that overlap the rows or one another return
 * ARIMA_E_INVALID_ARG. Lags are served 8 at a time: every further 8 cost one more pass pair over the rows.     */
int arima_diagnostics_batch(arima_handle *h, const double *rows, int64_t n_series, int32_t T, int32_t max_lag,
                            double *acf_out, double *dw_out, double *lb_stat_out, double *lb_pvalue_out);
/* Same, device-resident: d_rows N x T (row stride ld >= T, else ARIMA_E_INVALID_ARG), device outputs */
int arima_diagnostics_batch_device(arima_handle *h, const double *d_rows, int64_t n_series, int32_t T, int64_t ld,
                                   int32_t max_lag, double *d_acf_out, double *d_dw_out, double *d_lb_stat_out,
                                   double *d_lb_pvalue_out, void *stream);
/* The diagnostics of the residuals of every series under its model, without handing N x T residuals to the caller:
 * arima_remove_effects_batch into a workspace slice owned by the handle ("diag_slice_bytes"), then the diagnostics
 * of that slice, slice by slice, so device memory stays bounded whatever N is. Every order the effects entry points
 * accept; coef N x k. Bit-identical to arima_diagnostics_batch over arima_remove_effects_batch's output.         */
int arima_residual_diagnostics_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                                     int32_t p, int32_t d, int32_t q, int32_t include_intercept, const double *coef,
                                     int32_t max_lag, double *acf_out, double *dw_out, double *lb_stat_out,
                                     double *lb_pvalue_out);
int arima_residual_diagnostics_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T,
                                            int64_t ld, int32_t p, int32_t d, int32_t q, int32_t include_intercept,
                                            const double *d_coef, int32_t max_lag, double *d_acf_out,
                                            double *d_dw_out, double *d_lb_stat_out, double *d_lb_pvalue_out,
                                            void *stream);
/* ---- regressions over a regressor matrix: AutoregressionX, bgtest, bptest over a batch --------------------------- *
 * One computation, commons-math3 OLSMultipleLinearRegression (QR at threshold 0) over a design that is not made only
 * of a series' own lags, in the reference's arithmetic and order: coefficients, predictions and the test statistics
 * are bit-identical to tests/regress_ref.py; the p-values restate commons' chi-squared tail (csrc/arima_chisq.hpp)
 * and agree with it to a tolerance.
 * xreg / factors: per series n_xcols rows of T values, the column-major DenseMatrix(T, k) of the reference.
 * x_series_stride (elements): 0 = one matrix shared by every series, else the distance between two series' matrices,
 * at least n_xcols * T. n_xcols == 0 is legal for the arx entry points (xreg may then be NULL).
 * AutoregressionX.fitModel(y, x, yMaxLag, xMaxLag, includeOriginalX, noIntercept) (AutoregressionX.scala:48-92): with
 * maxLag = max(yMaxLag, xMaxLag) there are R = T - maxLag rows; row r is time t = r + maxLag with the predictors
 * y(t-1) .. y(t-yMaxLag), then for every x column in order x_c(t-1) .. x_c(t-xMaxLag), then, with includeOriginalX,
 * x_0(t) .. x_{k-1}(t); K = arima_arx_num_coef of them. coef_out N x (1 + K) = (c, coefficients), c = 0.0 under
 * no_intercept. status_out N carries what the reference throws, per series: ARIMA_ST_SERIES_TOO_SHORT (R < 0),
 * ARIMA_ST_NO_DATA (R == 0, or no column at all), ARIMA_ST_NOT_ENOUGH_DATA (K + 1 > R), ARIMA_ST_SINGULAR (an rDiag
 * of the QR exactly 0); a failed series has NaN outputs and never aborts the batch. NaN and Inf propagate as in the
 * JVM (status OK).
 * ARXModel.predict (:117-130): out N x (T - maxLag), results(r) = c then += value * coefficients(col) in column
 * order; coef N x (1 + K) as arima_arx_fit_batch writes it. T < maxLag returns ARIMA_E_INVALID_ARG.
 * bgtest(residuals, factors, maxLag) (TimeSeriesStatisticalTests.scala:276-288): rows t = maxLag .. T-1 of
 * [factors(t, .), u(t-1) .. u(t-maxLag)] against u(t), with an intercept; stat = (T - maxLag) * R^2, p-value its
 * chi-squared(maxLag) upper tail. max_lag < 1 returns ARIMA_E_INVALID_ARG (ChiSquaredDistribution(0) throws).
 * bptest(residuals, factors) (:320-329): T rows of factors(t, .) against u(t) * u(t), with an intercept;
 * stat = T * R^2, df = n_xcols. n_xcols < 1 returns ARIMA_E_INVALID_ARG. R^2 is calculateRSquared of commons-math3
 * 3.4.1: 1 - RSS / TSS, TSS by SecondMoment's running update (an unpinned reading). A failed series
 * has NaN statistic and p-value and its status as above.
 * Negative lags or column counts, T < 0 and an x_series_stride in (0, n_xcols * T) return ARIMA_E_INVALID_ARG; more
 * than 64 design columns (the ones column included) return ARIMA_E_UNSUPPORTED; N == 0 returns ARIMA_OK and writes
 * nothing. Every output is required; outputs that overlap an input or one another return ARIMA_E_INVALID_ARG. The
 * design of a slice of series lives in a workspace owned by the handle ("regress_slice_bytes"; 0, the default, = the
 * rule of "diag_slice_bytes"; slices are whole blocks of 64 series and results never depend on their size).        */
int arima_arx_num_coef(int32_t n_xcols, int32_t y_max_lag, int32_t x_max_lag, int32_t include_original_x);
int arima_arx_fit_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T, const double *xreg,
                        int64_t x_series_stride, int32_t n_xcols, int32_t y_max_lag, int32_t x_max_lag,
                        int32_t include_original_x, int32_t no_intercept, double *coef_out, int32_t *status_out);
int arima_arx_predict_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T, const double *xreg,
                            int64_t x_series_stride, int32_t n_xcols, int32_t y_max_lag, int32_t x_max_lag,
                            int32_t include_original_x, const double *coef, double *out);
int arima_bgtest_batch(arima_handle *h, const double *residuals, int64_t n_series, int32_t T, const double *factors,
                       int64_t x_series_stride, int32_t n_xcols, int32_t max_lag, double *stat_out,
                       double *pvalue_out, int32_t *status_out);
int arima_bptest_batch(arima_handle *h, const double *residuals, int64_t n_series, int32_t T, const double *factors,
                       int64_t x_series_stride, int32_t n_xcols, double *stat_out, double *pvalue_out,
                       int32_t *status_out);
/* Same, device-resident: d_series / d_residuals N x T (row stride ld >= T, else ARIMA_E_INVALID_ARG), device
 * regressors and outputs; d_out of the prediction N x (T - maxLag) with row stride ld_out >= T - maxLag            */
int arima_arx_fit_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T, int64_t ld,
                               const double *d_xreg, int64_t x_series_stride, int32_t n_xcols, int32_t y_max_lag,
                               int32_t x_max_lag, int32_t include_original_x, int32_t no_intercept,
                               double *d_coef_out, int32_t *d_status_out, void *stream);
int arima_arx_predict_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T, int64_t ld,
                                   const double *d_xreg, int64_t x_series_stride, int32_t n_xcols, int32_t y_max_lag,
                                   int32_t x_max_lag, int32_t include_original_x, const double *d_coef, double *d_out,
                                   int64_t ld_out, void *stream);
int arima_bgtest_batch_device(arima_handle *h, const double *d_residuals, int64_t n_series, int32_t T, int64_t ld,
                              const double *d_factors, int64_t x_series_stride, int32_t n_xcols, int32_t max_lag,
                              double *d_stat_out, double *d_pvalue_out, int32_t *d_status_out, void *stream);
int arima_bptest_batch_device(arima_handle *h, const double *d_residuals, int64_t n_series, int32_t T, int64_t ld,
                              const double *d_factors, int64_t x_series_stride, int32_t n_xcols, double *d_stat_out,
                              double *d_pvalue_out, int32_t *d_status_out, void *stream);
/* ---- RegressionARIMA.fitModel("cochrane-orcutt") over a batch (RegressionARIMA.scala:83-176) ---------------------- *
 * A regression of y on the regressor matrix with an intercept and AR(1) errors, by the iterated Cochrane-Orcutt
 * procedure, in the reference's arithmetic and order: every output is bit-identical to tests/regarima_ref.py.
 * series N x T; xreg and x_series_stride as for the arx entry points (per series n_xcols rows of T values, 0 = shared).
 * Per series: OLS of y on [1, X] (the QR above); while the Durbin-Watson statistic of the last regression's residuals
 * is outside (2 - 0.05, 2 + 0.05): rho = the no-intercept slope of res(t + 1) on res(t) (SimpleRegression(false));
 * OLS of y(t) - rho y(t-1) on [1, X(t, .) - rho X(t-1, .)] over T - 1 rows; beta(0) /= 1 - rho; res = y - (X beta +
 * beta(0)); until max_iter iterations have run or two successive rho differ by at most 0.001. SimpleRegression's sums
 * and dgemv's order are unpinned readings.
 * coef_out N x (1 + n_xcols) = regressionCoeff (intercept first); rho_out N = arimaCoeff(0), 0.0 for a series that
 * never iterated (arimaOrders is (1, 0, 0)); n_iter_out N (nullable): the iterations run, also for a failed series.
 * status_out N carries what the reference throws, per series: ARIMA_ST_NO_DATA (T == 0), ARIMA_ST_NOT_ENOUGH_DATA
 * (n_xcols + 1 > T at the first regression, n_xcols + 1 > T - 1 at a transformed one), ARIMA_ST_SINGULAR (an rDiag of
 * either QR exactly 0); a failed series has NaN coef and rho and never aborts the batch. NaN and Inf propagate as in
 * the JVM: a NaN rho gives NaN coefficients with status OK, and the NaN Durbin-Watson statistic ends the loop.
 * max_iter < 1 (the reference throws on every path), n_xcols < 1, T < 0 and an x_series_stride in (0, n_xcols * T)
 * return ARIMA_E_INVALID_ARG; more than 64 design columns (the ones column included) return ARIMA_E_UNSUPPORTED;
 * N == 0 returns ARIMA_OK and writes nothing. Outputs that overlap an input or one another return
 * ARIMA_E_INVALID_ARG. The whole iteration of a series runs in one kernel; a slice of series needs about
 * (2 n_xcols + 3) T doubles each in the workspace of "regress_slice_bytes", and results never depend on the slices. */
int arima_regarima_co_fit_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                                const double *xreg, int64_t x_series_stride, int32_t n_xcols, int32_t max_iter,
                                double *coef_out, double *rho_out, int32_t *n_iter_out, int32_t *status_out);
/* Same, device-resident: d_series N x T (row stride ld >= T, else ARIMA_E_INVALID_ARG)                           */
int arima_regarima_co_fit_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T,
                                       int64_t ld, const double *d_xreg, int64_t x_series_stride, int32_t n_xcols,
                                       int32_t max_iter, double *d_coef_out, double *d_rho_out,
                                       int32_t *d_n_iter_out, int32_t *d_status_out, void *stream);
/* ---- ARIMAX.fitModel and ARIMAXModel.forecast over a batch (ARIMAX.scala:59-161, :201-256) ------------------------ *
 * An ARIMA(p, d, q) with exogenous regressors, restated with the reference's quirks: every output is bit-identical to
 * tests/arimax_ref.py.
 * Coefficients: K' = arima_arimax_num_coef = 1 + p + q + nX, nX = n_xcols * xreg_max_lag + (include_original_xreg ?
 * n_xcols : 0): (intercept slot, AR, MA, xreg). Slot 0 exists without an intercept too (it then starts at 0.0).
 * Fit. series N x T; xreg and x_series_stride as for the arx entry points (per series n_xcols rows of T values, 0 =
 * shared). Without user_init the start point is: AutoregressionX.fitModel, always with an intercept, of the
 * UNDIFFERENCED series on the matrix differenced d times as one vector of n_xcols * T values (yMaxLag = p, xMaxLag =
 * xreg_max_lag); Hannan-Rissanen(p, q) on the differenced series, whose last q values go between the AR and the xreg
 * part. The first exception wins: the ARX status, then Hannan-Rissanen's. user_init (N x K', nullable) skips both.
 * The optimizer is ARIMA's css-cgd over all K' coordinates: the objective and gradient read the first I + p + q of
 * them in ARIMA's layout (without an intercept slot 0 is read as the first AR coefficient), the others are inert but
 * count in the restart period and come back in coef_out. The handle's "smear" option governs the gradient as for ARIMA.
 * coef_out N x K', ll_out N (logLikelihoodCSSARMA at coef_out), status_out N (ARIMA_ST_*; a failed series has NaN
 * coef and ll and never aborts the batch), n_eval_out / n_grad_out N, nullable (the reference's counters).
 * Forecast. ARIMAXModel.forecast(ts, xreg): xreg per series n_xcols columns of n_future values (x_series_stride 0 =
 * shared, else at least n_xcols * n_future); coef N x K'; out N x T: the LAST T of the T + n_future fitted and
 * forecast values (`results.drop(nFuture)`). The coefficients are read at offset 1 whatever include_intercept says,
 * and of xreg only column n_xcols - 1 reaches the output, times coefficient p + q + n_xcols (an assignment in the
 * reference's sum). Shapes the reference throws for are ARIMA_E_INVALID_ARG: max(p, q) == 0, T < d, and with
 * R = max(p, q) + max(n_future - d, 0): R < xreg_max_lag, or R - xreg_max_lag > max(p, q) + T - d. Every buffer is
 * required, xreg also when n_future == 0 (nothing is read through it then).
 * n_xcols < 1, negative orders, lags, T or n_future and an x_series_stride in (0, one matrix) return
 * ARIMA_E_INVALID_ARG; p or q > 20, d > 16, K' > 41 and (d + 2) T + n_future > 2^31 - 1 return
 * ARIMA_E_UNSUPPORTED; N == 0 returns ARIMA_OK and writes nothing. Outputs that overlap an input or one another return ARIMA_E_INVALID_ARG. A slice of series of a fit needs
 * about (K' - q + 1) (T - max(p, xreg_max_lag)) + T doubles each (and n_xcols * T more with per-series regressors) in
 * the workspace of "regress_slice_bytes"; results never depend on the slices.                                        */
int arima_arimax_num_coef(int32_t n_xcols, int32_t p, int32_t q, int32_t xreg_max_lag, int32_t include_original_xreg);
int arima_arimax_fit_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T, const double *xreg,
                           int64_t x_series_stride, int32_t n_xcols, int32_t p, int32_t d, int32_t q,
                           int32_t xreg_max_lag, int32_t include_original_xreg, int32_t include_intercept,
                           const double *user_init, double *coef_out, double *ll_out, int32_t *status_out,
                           int32_t *n_eval_out, int32_t *n_grad_out);
int arima_arimax_forecast_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T, const double *xreg,
                                int64_t x_series_stride, int32_t n_xcols, int32_t n_future, int32_t p, int32_t d,
                                int32_t q, int32_t xreg_max_lag, int32_t include_original_xreg,
                                int32_t include_intercept, const double *coef, double *out);
/* Same, device-resident: d_series N x T (row stride ld >= T, else ARIMA_E_INVALID_ARG), d_out N x T with row stride
 * ld_out >= T                                                                                                       */
int arima_arimax_fit_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T, int64_t ld,
                                  const double *d_xreg, int64_t x_series_stride, int32_t n_xcols, int32_t p, int32_t d,
                                  int32_t q, int32_t xreg_max_lag, int32_t include_original_xreg,
                                  int32_t include_intercept, const double *d_user_init, double *d_coef_out,
                                  double *d_ll_out, int32_t *d_status_out, int32_t *d_n_eval_out,
                                  int32_t *d_n_grad_out, void *stream);
int arima_arimax_forecast_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T, int64_t ld,
                                       const double *d_xreg, int64_t x_series_stride, int32_t n_xcols,
                                       int32_t n_future, int32_t p, int32_t d, int32_t q, int32_t xreg_max_lag,
                                       int32_t include_original_xreg, int32_t include_intercept, const double *d_coef,
                                       double *d_out, int64_t ld_out, void *stream);
/* ARIMAModel.isStationary / isInvertible (ARIMA.scala:777-815) for N coefficient rows, flags_out N */
int arima_model_flags_batch(arima_handle *h, const double *coef, int64_t n_series, int32_t p, int32_t q,
                            int32_t include_intercept, uint8_t *flags_out);

/* ---- order search (BASELINE config C5; ARIMA.autoFit's selection rule, ARIMA.scala:280-375)
 * Fits every (d, p, q, intercept) with d in [0,max_d], p in [0,max_p], q in [0,max_q] and intercept per
 * intercept_mode (0: without, 1: with, 2: both), in that lexicographic order, and keeps per series the fit
 * with the smallest approxAIC (ARIMA.scala:826-830) among those that returned normally and are stationary and
 * invertible (the isStationary && isInvertible filter, ARIMA.scala:342); ties keep the first.
 * order_out N x 4 = (p, d, q, intercept), -1s when no candidate qualified; coef_out N x 11 (zero-padded, NaN
 * when none); aic_out N (+inf when none). Host buffers; the _device variant takes device pointers.          */
int arima_order_search_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                             int32_t max_p, int32_t max_d, int32_t max_q, int32_t intercept_mode, int32_t method,
                             int32_t *order_out, double *coef_out, double *aic_out);
int arima_order_search_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T,
                                    int64_t ld, int32_t max_p, int32_t max_d, int32_t max_q,
                                    int32_t intercept_mode, int32_t method, int32_t *d_order_out,
                                    double *d_coef_out, double *d_aic_out, void *stream);

/* ---- ARIMA.autoFit over a batch (ARIMA.scala:280-375; python/sparkts/models/ARIMA.py:25-60 `autofit`) --------- *
 * Per series: d = the first of 0..max_d whose differencesOfOrderD(ts, d) (NOT dropped) passes kpsstest(_, "c") at 5 %
 * (TimeSeriesStatisticalTests.scala:369-395); then findBestARMAModel's stepwise walk over (p, q, intercept) on that
 * differenced series with css-cgd fits, a css-bobyqa retry where css-cgd throws in the optimizer (fitTryBothStrategies,
 * ARIMA.scala:315-319) (intercept only for d <= 1; the neighbourhood never changes q -- the
 * reference's quirks, ARIMA.scala:298-300, :356-366), keeping the first minimum approxAIC among stationary and
 * invertible fits. max_p <= 8 (any max_q: the walk only meets q <= 2), any series length (KPSS lags above 32 take
 * one pass per lag). order_out N x 4 = (p, d, q, intercept) (-1s when the series has no model),
 * coef_out N x 11 (zero-padded; NaN when none), aic_out N (+inf when none), status_out N: ARIMA_ST_OK,
 * ARIMA_ST_NOT_STATIONARY, ARIMA_ST_NO_MODEL, or the KPSS regression's shape status (T <= 1). n_fits_out (nullable): candidate fits the walk ran for the series.        */
int arima_autofit_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T, int32_t max_p,
                        int32_t max_d, int32_t max_q, int32_t *order_out, double *coef_out, double *aic_out,
                        int32_t *status_out, int32_t *n_fits_out);
int arima_autofit_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T, int64_t ld,
                               int32_t max_p, int32_t max_d, int32_t max_q, int32_t *d_order_out,
                               double *d_coef_out, double *d_aic_out, int32_t *d_status_out, int32_t *d_n_fits_out,
                               void *stream);
/* TimeSeriesStatisticalTests.kpsstest(ts, "c") (TimeSeriesStatisticalTests.scala:369-393) per series: stat_out N,
 * status_out N (ARIMA_ST_OK, or the OLS shape status for T <= 1). Host buffers.                                  */
int arima_kpss_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T, double *stat_out,
                     int32_t *status_out);

/* ---- the small model families: EWMA (EWMA.scala) and GARCH(1,1) (GARCH.scala) over a batch --------------------- *
 * Both fits run commons-math3's Fletcher-Reeves NonLinearConjugateGradientOptimizer with its default LineSearch,
 * SimpleValueChecker(1e-6, 1e-6), MaxIter(10000), MaxEval(10000), one lane per series (csrc/cg_small.hpp,
 * csrc/arima_models.hip); results are the reference's arithmetic in its operation order (tests/smallfit_ref.py
 * restates it). status_out: ARIMA_ST_OK, _MAX_EVAL, _BRACKET_MAX_EVAL, _MAX_ITER or _BAD_INTERVAL (the exceptions the
 * optimizer can throw); a failed series has NaN parameters and a NaN objective. n_eval_out / n_grad_out (nullable):
 * the reference's evaluation and gradient counts.
 *
 * EWMA.fitModel (EWMA.scala:45-69): one parameter, `smoothing`, from [0.94], GoalType.MINIMIZE of EWMAModel.sse.
 * GARCH.fitModel (GARCH.scala:33-53): (omega, alpha, beta) from [.2, .2, .2]. No GoalType is passed, so commons
 *   MAXIMISES GARCHModel.logLikelihood. GARCHModel.gradient returns (alpha, beta, omega) halves (:114) and the
 *   optimizer applies component 0 to omega, 1 to alpha, 2 to beta: that mismatch is the reference's and is reproduced,
 *   not repaired -- a drop-in returns what spark-ts returns (on rows far from the start it leaves the positive region).
 *   Nothing is special-cased: a negative h gives NaN through the log, overflow gives Inf, as Java's doubles do.
 *
 * Argument rules (all entry points of this section): fits and the objective / gradient building blocks with T == 0
 * return ARIMA_E_INVALID_ARG (EWMA reads ts(0)); T >= 1 runs the reference's arithmetic whatever it yields. Effects
 * with N == 0 or T == 0 return ARIMA_OK and write nothing. ld < T (ld_out < T) returns ARIMA_E_INVALID_ARG. Any
 * overlap of an output with an input or another output returns ARIMA_E_INVALID_ARG -- there is no in-place form
 * (EWMA's remove reads ts(i - 1) after arr(i - 1) is written). Nothing is written past column T of a row.
 * Device variants are asynchronous on the caller's stream and ordered on the handle like every other call.          */
int arima_ewma_fit_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                         double *smoothing_out, double *sse_out, int32_t *status_out, int32_t *n_eval_out,
                         int32_t *n_grad_out);
int arima_ewma_fit_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T, int64_t ld,
                                double *d_smoothing_out, double *d_sse_out, int32_t *d_status_out,
                                int32_t *d_n_eval_out, int32_t *d_n_grad_out, void *stream);
/* coef_out N x 3 = (omega, alpha, beta); ll_out N: logLikelihood at coef_out */
int arima_garch_fit_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T, double *coef_out,
                          double *ll_out, int32_t *status_out, int32_t *n_eval_out, int32_t *n_grad_out);
int arima_garch_fit_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T, int64_t ld,
                                 double *d_coef_out, double *d_ll_out, int32_t *d_status_out, int32_t *d_n_eval_out,
                                 int32_t *d_n_grad_out, void *stream);
/* Building blocks (host buffers): the fit's own pass routine at caller-given parameters, one model per series.
 * EWMAModel.sse (EWMA.scala:81-96) / gradient (:102-123, the reference's 2 * dJda); smoothing N, out N.
 * GARCHModel.logLikelihood (GARCH.scala:82-88) / gradient (:96-115); coef N x 3 = (omega, alpha, beta), ll_out N,
 * grad_out N x 3 in the reference's RETURNED order (alpha, beta, omega). */
int arima_ewma_sse_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T, const double *smoothing,
                         double *sse_out);
int arima_ewma_gradient_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                              const double *smoothing, double *grad_out);
int arima_garch_loglik_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T, const double *coef,
                             double *ll_out);
int arima_garch_gradient_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T, const double *coef,
                               double *grad_out);
/* The TimeSeriesModel pairs, N x T in, N x T out, one model per series (smoothing N / coef N x 3).
 * EWMAModel.removeTimeDependentEffects (EWMA.scala:125-133; reads ts(i - 1), no recursion) and
 * addTimeDependentEffects (:135-143; the recursion on dest(i - 1)); GARCHModel's (GARCH.scala:131-162). */
int arima_ewma_remove_effects_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                                    const double *smoothing, double *out);
int arima_ewma_add_effects_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                                 const double *smoothing, double *out);
int arima_garch_remove_effects_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                                     const double *coef, double *out);
int arima_garch_add_effects_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                                  const double *coef, double *out);
int arima_ewma_remove_effects_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T,
                                           int64_t ld, const double *d_smoothing, double *d_out, int64_t ld_out,
                                           void *stream);
int arima_ewma_add_effects_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T,
                                        int64_t ld, const double *d_smoothing, double *d_out, int64_t ld_out,
                                        void *stream);
int arima_garch_remove_effects_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T,
                                            int64_t ld, const double *d_coef, double *d_out, int64_t ld_out,
                                            void *stream);
int arima_garch_add_effects_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T,
                                         int64_t ld, const double *d_coef, double *d_out, int64_t ld_out,
                                         void *stream);
/* ---- ARGARCH (GARCH.scala:56-70, 198-260), ARModel's pair (Autoregression.scala:56-96) and the GARCH samples ------ *
 * The argument rules of the section above hold for every entry point here.
 *
 * ARGARCH.fitModel (GARCH.scala:63-69): Autoregression.fitModel(ts) -- AR(1) with an intercept, the arithmetic of
 * arima_fit_batch(p = 1, d = 0, q = 0, intercept), bit for bit -- then GARCH.fitModel on the residuals
 * r(0) = ts(0) - c, r(i) = (ts(i) - c) - ts(i - 1) * phi (ARModel.removeTimeDependentEffects). The residuals are formed
 * inside the GARCH passes from the raw rows; no N x T residual buffer exists on the device.
 * coef_out N x 5 = (c, phi, omega, alpha, beta); ll_out N: GARCHModel.logLikelihood of the residuals at the fitted
 * parameters. status_out: the AR stage's status when it is not ARIMA_ST_OK (ARIMA_ST_NO_DATA at T = 1,
 * _NOT_ENOUGH_DATA at T = 2, _SINGULAR for a constant row) with both counters 0, else the GARCH stage's. A series
 * that failed in either stage has five NaN coefficients and a NaN ll (the reference throws and returns no model).  */
int arima_argarch_fit_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T, double *coef_out,
                            double *ll_out, int32_t *status_out, int32_t *n_eval_out, int32_t *n_grad_out);
int arima_argarch_fit_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T, int64_t ld,
                                   double *d_coef_out, double *d_ll_out, int32_t *d_status_out, int32_t *d_n_eval_out,
                                   int32_t *d_n_grad_out, void *stream);
/* ARGARCHModel.removeTimeDependentEffects / addTimeDependentEffects (GARCH.scala:205-236); coef N x 5 */
int arima_argarch_remove_effects_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                                       const double *coef, double *out);
int arima_argarch_add_effects_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T,
                                    const double *coef, double *out);
int arima_argarch_remove_effects_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T,
                                              int64_t ld, const double *d_coef, double *d_out, int64_t ld_out,
                                              void *stream);
int arima_argarch_add_effects_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T,
                                           int64_t ld, const double *d_coef, double *d_out, int64_t ld_out,
                                           void *stream);
/* ARModel.removeTimeDependentEffects / addTimeDependentEffects (Autoregression.scala:60-90) at order p; coef
 * N x (1 + p) = (c, phi_1 .. phi_p) per series. Step i uses only the lags that exist (i - j - 1 >= 0), which differs
 * from ARIMAModel's pair with d = q = 0. p < 1 returns ARIMA_E_INVALID_ARG, p > 20 ARIMA_E_UNSUPPORTED.
 * ARModel.sample(n, rand) is add_effects of n gaussians (computed out of place it yields the same values).         */
int arima_ar_remove_effects_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T, int32_t p,
                                  const double *coef, double *out);
int arima_ar_add_effects_batch(arima_handle *h, const double *series, int64_t n_series, int32_t T, int32_t p,
                               const double *coef, double *out);
int arima_ar_remove_effects_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T,
                                         int64_t ld, int32_t p, const double *d_coef, double *d_out, int64_t ld_out,
                                         void *stream);
int arima_ar_add_effects_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T,
                                      int64_t ld, int32_t p, const double *d_coef, double *d_out, int64_t ld_out,
                                      void *stream);
/* GARCHModel.sample (GARCH.scala:164-185; coef N x 3) / ARGARCHModel.sample (:238-259; coef N x 5) with the gaussians
 * drawn by the caller: z N x T, z(i, t) = the t-th nextGaussian() of series i; out N x T. As in the reference out(i, 0)
 * is 0.0 and z(i, 0) only feeds the variance of step 1. N == 0 or T == 0 writes nothing.                            */
int arima_garch_sample_batch(arima_handle *h, const double *z, int64_t n_series, int32_t T, const double *coef,
                             double *out);
int arima_argarch_sample_batch(arima_handle *h, const double *z, int64_t n_series, int32_t T, const double *coef,
                               double *out);
int arima_garch_sample_batch_device(arima_handle *h, const double *d_z, int64_t n_series, int32_t T, int64_t ld,
                                    const double *d_coef, double *d_out, int64_t ld_out, void *stream);
int arima_argarch_sample_batch_device(arima_handle *h, const double *d_z, int64_t n_series, int32_t T, int64_t ld,
                                      const double *d_coef, double *d_out, int64_t ld_out, void *stream);

/* Counters of the last EWMA / GARCH / ARGARCH fit call on the handle (waits for its device work; ARGARCH: its GARCH
 * stage, whose rounds equal those of a GARCH fit of the residual rows). The fit kernel runs one wave
 * per 64 series in rounds: one joint objective + gradient pass over the wave's rows per round, finished lanes masked. */
typedef struct arima_model_fit_stats {
    int64_t n_series;
    int64_t wave_passes;       /* rounds summed over the waves                                        */
    int64_t lane_passes;       /* live lanes summed over those rounds (= passes over a series)         */
    int64_t max_wave_passes;   /* the rounds of the slowest wave                                       */
} arima_model_fit_stats;
int arima_get_last_model_fit_stats(arima_handle *h, arima_model_fit_stats *out);

/* ---- synthetic workload generator (ARIMAModel.sample semantics, ARIMA.scala:655-678) ---------------- *
 * Writes N x T series (row stride ld) into device memory: per-series coefficients = base +/- U(0, jitter)
 * (redrawn until stationary and invertible), Philox4x32-10 + Box-Muller N(0,1) noise keyed by (seed,
 * first_series + i, t). Deterministic for a given (seed, global series id) whatever the sharding.           */
int arima_sample_batch_device(arima_handle *h, double *d_series, int64_t n_series, int32_t T, int64_t ld,
                              int32_t p, int32_t d, int32_t q, int32_t include_intercept,
                              const double *base_coef, double jitter, uint64_t seed, int64_t first_series,
                              void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SPARKTS_ARIMA_H */
