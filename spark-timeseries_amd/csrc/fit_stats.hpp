// fit_stats.hpp — "the stats of the last fit" as pure functions: the names of the fit kernel's counter words the host
// reads, the one table from counter word to arima_fit_stats member, the flops formula, a fit's stats
// from its counters, the order search's per-fit accumulation (k_search_acc's body) and its stats from the lanes' sums,
// and the sum of one stats value into another. No HIP headers on the host: a CPU program includes this file and
// compares the functions with the bodies they replaced (tests/sim/fitstats_sim.cpp). arima_runtime.cpp reads the
// events and the pinned counter copies and keeps no second copy of the mapping or of the formula.
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/sparkts_arima.h"

#ifdef __HIPCC__
#define STS_HD __host__ __device__
#else
#define STS_HD
#endif

namespace sts {
namespace stats {

// Counter words of the fit kernels (k_cg_fit's ctl[], arima_kernels_impl.hpp; the kernels keep their literal indices)
enum CtlWord : int {
    kCtlFPasses = 1, kCtlGPasses = 2, kCtlWaveFPasses = 3, kCtlWaveGPasses = 4, kCtlNEval = 5, kCtlNGrad = 6,
    kCtlSpecHits = 7, kCtlWaveMultiPasses = 8, kCtlSpecChains = 9,
    // STS_TIMING builds: F-pass, G-pass, advance, select cycles (summed over waves), the kernel's last end and first
    // start, the per-wave time after the batch drained
    kCtlTimeF = 10, kCtlTimeG = 11, kCtlTimeAdvance = 12, kCtlTimeSelect = 13, kCtlTimeEnd = 14, kCtlTimeStart = 15,
    kCtlTimeDrained = 16,
    kCtlRidePasses = 18, kCtlExpressSeries = 23, kCtlExpressFPasses = 24, kCtlExpressGPasses = 25,
    kCtlFault = 26, kCtlFaultInfo = 27, kCtlFaultLast = 31,   // the watchdog's record: code, five info words
    kCtlSeriesDone = 32, kCtlExpressPitPasses = 33, kCtlExpressPitSweeps = 34, kCtlExpressPitGPasses = 35,
    kCtlWaveChains = 36, kCtlLowUtilPasses = 37, kCtlTimeStep = 38, kCtlTimeRefill = 39, kCtlMergeSeries = 41,
    kCtlMergeWaves = 42,
    kCtlWords = 48
};
// The kernels' words after that block. The functions below take the 48-word block and the lane sums built on it
// (tests/sim/fitstats_sim.cpp compares them, every word and every stats member, with the bodies they replaced), so a
// later counter is carried beside it: with_ext_counters for a fit's counter copy of kCtlWordsExt words,
// search_acc_ext for the order search's lanes, and acc_stats for sums.
constexpr int kCtlSkippedG = kCtlWords;       // gradient evaluations counted without a pass (cg_lane.hpp SKIPG)
constexpr int kCtlWordsExt = kCtlWords + 1;
constexpr int kFaultWords = kCtlFaultLast - kCtlFault + 1;
STS_HD inline bool fault_word(int i) { return i >= kCtlFault && i <= kCtlFaultLast; }

// The one mapping from counter word to stats member. The first kSummedFields entries are what a sum carries (the
// order search's lane sums, acc_stats); the two STS_TIMING words after them are read for a single fit only, so sliced
// fits, host fits and searches leave them zero.
struct CtlField {
    int word;
    int64_t arima_fit_stats::*member;
};
constexpr CtlField kCtlFields[] = {
    {kCtlFPasses, &arima_fit_stats::f_passes},
    {kCtlGPasses, &arima_fit_stats::g_passes},
    {kCtlWaveFPasses, &arima_fit_stats::wave_f_passes},
    {kCtlWaveGPasses, &arima_fit_stats::wave_g_passes},
    {kCtlNEval, &arima_fit_stats::n_eval},
    {kCtlNGrad, &arima_fit_stats::n_grad},
    {kCtlSpecHits, &arima_fit_stats::spec_hits},
    {kCtlWaveMultiPasses, &arima_fit_stats::wave_multi_passes},
    {kCtlSpecChains, &arima_fit_stats::spec_chains},
    {kCtlRidePasses, &arima_fit_stats::ride_passes},
    {kCtlExpressSeries, &arima_fit_stats::express_series},
    {kCtlExpressFPasses, &arima_fit_stats::express_f_passes},
    {kCtlExpressGPasses, &arima_fit_stats::express_g_passes},
    {kCtlSeriesDone, &arima_fit_stats::series_done},
    {kCtlExpressPitPasses, &arima_fit_stats::express_pit_passes},
    {kCtlExpressPitSweeps, &arima_fit_stats::express_pit_sweeps},
    {kCtlExpressPitGPasses, &arima_fit_stats::express_pit_g_passes},
    {kCtlWaveChains, &arima_fit_stats::wave_chains},
    {kCtlLowUtilPasses, &arima_fit_stats::low_util_passes},
    {kCtlMergeSeries, &arima_fit_stats::merge_series},
    {kCtlMergeWaves, &arima_fit_stats::merge_waves},
    {kCtlTimeStep, &arima_fit_stats::diag_step_cycles},
    {kCtlTimeRefill, &arima_fit_stats::diag_refill_cycles},
};
constexpr int kAllFields = (int)(sizeof(kCtlFields) / sizeof(kCtlFields[0]));
constexpr int kSummedFields = kAllFields - 2;

inline void fields_from_counters(arima_fit_stats &st, const unsigned long long *cc, int fields) {
    for (int i = 0; i < fields; ++i) st.*kCtlFields[i].member = (int64_t)cc[kCtlFields[i].word];
    st.fault = (int64_t)cc[kCtlFault];
    for (int i = 0; i < kFaultWords - 1; ++i) st.fault_info[i] = (int64_t)cc[kCtlFaultInfo + i];
}

// Algorithmic flops of one fit: U*S*(2(p+q)+4) + G*S*(2(p+q)+4 + 2kq + 1+p+q + 2k) + W_HR, with
// U = distinct objective points evaluated by a pass (bulk objective passes, objective requests served by gradient
// passes, express objective passes, and the speculative points the optimizer then used) and G = gradient evaluations
// that ran a pass (bulk gradient passes without the objective riders, express ones). with_hr: count the two least
// squares of the Hannan-Rissanen init (W_HR). `sum` is the running total the fit is added to, term by term from the
// left as the search's accumulation always did (0.0 for a fit alone: exact, the first term is never negative). The
// build never contracts a*b+c, so host and device agree bit for bit.
STS_HD inline double fit_flops(double sum, int64_t N, int n, int p, int q, int I, double U, double G, bool with_hr) {
    const int k = I + p + q, M = p > q ? p : q, m = M + 1;
    const double S = n - M > 0 ? n - M : 0;
    const double ff = 2.0 * (p + q) + 4, fg = ff + 2.0 * k * q + 1 + p + q + 2.0 * k;
    const double whr = (double)N * (3.0 * (n - m > 0 ? n - m : 0) * (m + 1) * (m + 1) +
                                    3.0 * (n - 2 * M - 1 > 0 ? n - 2 * M - 1 : 0) * k * k +
                                    2.0 * (n - m > 0 ? n - m : 0) * m);
    return sum + U * S * ff + G * S * fg + (with_hr ? whr : 0.0);
}

// What turns the device counters of one fit (or slice, or host chunk) into arima_fit_stats
struct FitShape {
    bool valid = false;
    int64_t N = 0;
    int n = 0, p = 0, q = 0, I = 0;
    bool ar_only = false, user_init = false, cg = false;
    int64_t grid = 0, express = 0;
};
struct FitTimes {                   // elapsed ms between the fit's events
    double difference = 0, hr_init = 0, cg_fit = 0, total = 0;
};

// The stats of one finished fit from its shape, its counter copy and its elapsed times.
inline arima_fit_stats fit_stats(const FitShape &ps, const unsigned long long *cc, const FitTimes &t) {
    arima_fit_stats st{};
    if (!ps.valid) return st;
    const int64_t N = ps.N;
    const int p = ps.p, q = ps.q, I = ps.I, k = I + p + q;
    st.ms_difference = t.difference;
    st.ms_hr_init = t.hr_init;
    st.ms_cg_fit = t.cg_fit;
    st.ms_total = t.total;
    fields_from_counters(st, cc, kAllFields);
    // series the kernels wrote; the AR-only shortcut, user-uniform statuses and an empty fit write every series
    if (!ps.cg) st.series_done = N;
    st.diag[0] = (int64_t)cc[kCtlTimeF];
    st.diag[1] = (int64_t)cc[kCtlTimeG];
    st.diag[2] = (int64_t)cc[kCtlTimeAdvance];
    st.diag[3] = (int64_t)cc[kCtlTimeSelect];
    st.diag[4] = cc[kCtlTimeEnd] ? (int64_t)(cc[kCtlTimeEnd] - cc[kCtlTimeStart]) : 0;   // the kernel's span
    st.diag[5] = (int64_t)cc[kCtlTimeDrained];
    st.grid_blocks = ps.grid;
    st.express_blocks = ps.express;
    // HR passes: 2 per column of each of the two least squares, minus the norm pass of an intercept column (the
    // sum of ones needs no stream; arima_device.hpp ols_stage)
    const int m = (p > q ? p : q) + 1;
    if (ps.ar_only) st.hr_passes = N * (int64_t)(2 * (I + p) - I);
    else if (!ps.user_init) st.hr_passes = N * (int64_t)(2 * (1 + m) - 1 + 2 * k - I);
    const double U = (double)(st.f_passes + st.ride_passes + st.express_f_passes + st.spec_hits);
    const double G = (double)(st.g_passes - st.ride_passes + st.express_g_passes);
    // W_HR for every fit without user inits -- also the AR-only shortcut, which runs one OLS instead. The order
    // search (search_acc_fit) leaves it out for AR-only fits: the two callers differ, and stay as they were.
    st.flops = fit_flops(0.0, N, ps.n, p, q, I, U, G, !ps.user_init);
    st.n_series = N;
    return st;
}

// The same from the kernels' whole counter copy (kCtlWordsExt words): the members fed by the words after the block.
// The flops figure counts passes that ran, so a skipped gradient is in neither G nor the flops.
inline arima_fit_stats with_ext_counters(arima_fit_stats st, const FitShape &ps, const unsigned long long *cc) {
    if (ps.valid) st.skipped_g = (int64_t)cc[kCtlSkippedG];
    return st;
}

// One grid point's fit into its search lane's sums acc[kCtlWords + 1] (k_search_acc): every counter word, and the
// fit's flops (a double in the last word). cg = 0: the AR-only shortcut or a uniform status (no counters; every series
// written). The fault words are not summed: the lane keeps the first fault any of its fits recorded.
STS_HD inline void search_acc_fit(const unsigned long long *ctl, unsigned long long *acc, int64_t N, int n, int p,
                                  int q, int I, int cg) {
    for (int i = 0; i < kCtlWords; ++i)
        if (!fault_word(i)) acc[i] += ctl[i];
    if (acc[kCtlFault] == 0 && ctl[kCtlFault] != 0)
        for (int i = kCtlFault; i <= kCtlFaultLast; ++i) acc[i] = ctl[i];
    if (!cg) acc[kCtlSeriesDone] += (unsigned long long)N;
    const double U = (double)(ctl[kCtlFPasses] + ctl[kCtlRidePasses] + ctl[kCtlExpressFPasses] + ctl[kCtlSpecHits]);
    const double G = (double)(ctl[kCtlGPasses] - ctl[kCtlRidePasses] + ctl[kCtlExpressGPasses]);
    // W_HR unless AR-only (p > 0, q == 0: one OLS, not the Hannan-Rissanen init). fit_stats counts it there too.
    const bool ar_only = p > 0 && q == 0;
    double *fl = reinterpret_cast<double *>(acc + kCtlWords);
    *fl = fit_flops(*fl, N, n, p, q, I, U, G, !ar_only);
}

// The words after the block, of the same fit, into the lane's ext[kCtlWordsExt - kCtlWords] sums (k_search_acc), and
// the lanes' sums (lanes x that many words) into the search's stats
constexpr int kExtWords = kCtlWordsExt - kCtlWords;
STS_HD inline void search_acc_ext(const unsigned long long *ctl, unsigned long long *ext) {
    for (int i = 0; i < kExtWords; ++i) ext[i] += ctl[kCtlWords + i];
}
inline void search_stats_ext(arima_fit_stats &st, const unsigned long long *lane_ext, int lanes) {
    for (int j = 0; j < lanes; ++j) st.skipped_g += (int64_t)lane_ext[(size_t)j * kExtWords + (kCtlSkippedG - kCtlWords)];
}

// The stats of an order search from its lanes' sums (lanes x (kCtlWords + 1) words): n_fits = series x grid points,
// grid / express = the last css-cgd fit's launch, ms = the call's device time. No HR passes, phase times or
// STS_TIMING words.
inline arima_fit_stats search_stats(const unsigned long long *lane_acc, int lanes, int64_t n_fits, int64_t grid,
                                    int64_t express, double ms) {
    arima_fit_stats st{};
    unsigned long long w[kCtlWords] = {};
    for (int j = 0; j < lanes; ++j) {
        const unsigned long long *a = lane_acc + (size_t)j * (kCtlWords + 1);
        for (int i = 0; i < kCtlWords; ++i)
            if (!fault_word(i)) w[i] += a[i];
        if (w[kCtlFault] == 0 && a[kCtlFault] != 0)            // the first lane's recorded fault
            for (int i = kCtlFault; i <= kCtlFaultLast; ++i) w[i] = a[i];
        double f;
        memcpy(&f, a + kCtlWords, sizeof f);
        st.flops += f;
    }
    fields_from_counters(st, w, kSummedFields);
    st.n_series = n_fits;
    st.grid_blocks = grid;
    st.express_blocks = express;
    st.ms_cg_fit = ms;
    st.ms_total = ms;
    return st;
}

// a += s over slices or chunks: times, passes and flops add up; the launch shape is the last fit's, the fault record
// the first one's
inline void acc_stats(arima_fit_stats &a, const arima_fit_stats &s) {
    a.ms_difference += s.ms_difference;
    a.ms_hr_init += s.ms_hr_init;
    a.ms_cg_fit += s.ms_cg_fit;
    a.ms_total += s.ms_total;
    a.hr_passes += s.hr_passes;
    a.flops += s.flops;
    a.n_series += s.n_series;
    for (int i = 0; i < kSummedFields; ++i) a.*kCtlFields[i].member += s.*kCtlFields[i].member;
    a.skipped_g += s.skipped_g;
    a.grid_blocks = s.grid_blocks;
    a.express_blocks = s.express_blocks;
    if (!a.fault && s.fault) {
        a.fault = s.fault;
        for (int i = 0; i < kFaultWords - 1; ++i) a.fault_info[i] = s.fault_info[i];
    }
}

}  // namespace stats
}  // namespace sts
