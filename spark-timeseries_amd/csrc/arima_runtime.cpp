// arima_runtime.cpp — the C ABI (include/sparkts_arima.h) over the HIP kernels: one handle per device, a
// private stream, grow-only device workspaces, per-call HIP-event timing and aggregate pass counters.
//
// Call flow of arima_fit_batch_device (the drop-in for ARIMA.fitModel over one Spark partition,
// ARIMA.scala:79-116):
//   k_difference (differencesOfOrderD(ts, d).drop(d), :88)  ->  p>0 && q==0 ? k_ar_fit (:90-96)
//   : [k_hr_init (:99-103, unless user init)] -> k_cg_fit (fitWithCSSCGD, :105-109, :174-200)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sparkts_arima.h"
#include "arima_launch.hpp"
#include "fit_stats.hpp"
#include "host_plan.hpp"

namespace {

struct DevBuf {
    void *ptr = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t need) {
        if (need <= bytes) return ARIMA_OK;
        if (ptr) hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
        if (need == 0) return ARIMA_OK;
        if (hipMalloc(&ptr, need) != hipSuccess) return ARIMA_E_OOM;
        bytes = need;
        return ARIMA_OK;
    }
    void release() {
        if (ptr) hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    template <class T>
    T *as() const { return static_cast<T *>(ptr); }
};

constexpr int kNumEvents = 5;
using namespace sts::stats;                    // kCtlWords and the names of the fit kernel's counter words
static_assert(kCtlWordsExt == sts::kFitCtlWords && kCtlSkippedG == sts::kFitCtlSkippedG,
              "fit_stats.hpp names the words the launchers prepare");
using sts::FitOut;

// What arima_get_last_stats needs to turn the device counters of one fit (or slice, or host chunk) into
// arima_fit_stats. The fit entry points do not wait for the device (the `*_device` contract): the counters are copied
// to pinned host memory in stream order and the stats are computed when they are asked for (fit_stats.hpp).
struct FitRecord {
    hipEvent_t ev[kNumEvents] = {};           // start, after differencing, init, fit; (slots) after the counter copy
    unsigned long long *ctl_host = nullptr;   // pinned, kCtlWordsExt
    FitShape ps;
    int create() {
        for (auto &e : ev)
            if (!e && hipEventCreate(&e) != hipSuccess) return ARIMA_E_DEVICE;
        return ARIMA_OK;
    }
    void destroy() {
        for (auto &e : ev)
            if (e) hipEventDestroy(e);
    }
    // the record's stats once its last event has passed; it stays valid (the callers retire it)
    arima_fit_stats stats() const {
        if (!ps.valid) return arima_fit_stats{};
        float d = 0, i = 0, f = 0, t = 0;
        hipEventElapsedTime(&d, ev[0], ev[1]);
        hipEventElapsedTime(&i, ev[1], ev[2]);
        hipEventElapsedTime(&f, ev[2], ev[3]);
        hipEventElapsedTime(&t, ev[0], ev[3]);
        return with_ext_counters(fit_stats(ps, ctl_host, FitTimes{d, i, f, t}), ps, ctl_host);
    }
};

// Device workspace of one fit in flight: Hannan-Rissanen init, the fit kernel's counters and its express ring.
struct FitWs {
    DevBuf init, hr_status, ctl, xring, xready;
    // every workspace of a fit of N series with k parameters, before the first launch (a growing DevBuf frees, and
    // hipFree synchronises the device)
    int reserve(int64_t N, int k) {
        int rc = init.ensure((size_t)N * std::max(k, 1) * sizeof(double));
        if (rc == ARIMA_OK) rc = hr_status.ensure((size_t)N * sizeof(int32_t));
        if (rc == ARIMA_OK) rc = ctl.ensure(kCtlWordsExt * sizeof(unsigned long long));
        if (rc == ARIMA_OK) rc = xring.ensure(sts::kExpressRingBytes);
        if (rc == ARIMA_OK) rc = xready.ensure(sts::kExpressReadyBytes);
        return rc;
    }
};

// One lane of the order search's concurrent fits (arima_order_search_batch*): its own stream, workspace and
// candidate outputs. Fits of consecutive grid points run on different lanes, so the tail of one fit kernel (its
// slowest series) overlaps the next fits; the select steps stay in grid order on the call's stream.
struct SearchLane {
    hipStream_t stream = nullptr;
    hipEvent_t ev_fit = nullptr, ev_sel = nullptr;
    bool sel_recorded = false;
    FitWs ws;
    DevBuf coef, ll, status, neval, ngrad, flags;
    FitOut out() const {
        return {coef.as<double>(), ll.as<double>(), status.as<int32_t>(), neval.as<int32_t>(), ngrad.as<int32_t>(),
                flags.as<uint8_t>()};
    }
    DevBuf best_aic, best_order, best_coef;    // this lane's best candidate per series (merged at the end)
    // kCtlWords counter sums over the lane's fits + their flops (double), then the kExtWords sums of the later words
    DevBuf acc;
};

// A device fit larger than one slice (option "fit_slice_bytes" of differenced workspace; default 0 = 60 % of the free
// HBM over the fit contexts) runs as consecutive slices over the fit contexts: the workspaces stay bounded whatever
// the batch (C3's 8M series on one GPU), and the slices pipeline like consecutive calls. Every slice takes the next slot of a ring with
// its own fit record (timing events, pinned copy of the kernel counters), so the call's stats cover every slice. A
// slot is reused only once its previous slice's copy has landed (host check on its last event).
constexpr int kSliceSlots = 64;
struct SliceSlot {
    FitRecord rec;
    bool used = false;
};

enum class StatsFrom { kNone, kContext, kSlices, kSearch };
constexpr int kMaxSearchLanes = sts::kSearchMaxLanes;
constexpr int kMaxD = 16;
constexpr int kMaxPipeline = 8;
constexpr int64_t kBobyqaWaveMaxN = 4096;     // css-bobyqa fits up to this many series: a wave per series
using sts::plan::ByteSpan;

// One fit context: what a fit call needs for itself (stream, differenced-series workspace, HR init, kernel counters,
// timing events, pinned counter copy, host-path staging). Fit calls rotate over h->pipeline contexts, so with
// pipeline > 1 consecutive fits run concurrently and the tail of one fit kernel (its slowest series) overlaps the
// next fit's differencing, init and bulk work; a context is reused only after its previous call has finished.
// One device-fit call's caller buffers as byte ranges [lo, hi) (series rows and user inits read; the six outputs
// written) -- fit_pipeline > 1 hazard tracking
struct CallSpans {
    ByteSpan in[2], out[6];
};
constexpr int kInflightMax = 16;   // tracked calls per context; beyond, every later call waits for that context
struct Inflight {                  // the device-fit calls on one context that may not have finished yet
    CallSpans call[kInflightMax];
    hipEvent_t ev[kInflightMax] = {};   // each call's end (a hazard waits for exactly that call)
    int n = 0;
    bool overflow = false;
};

struct FitCtx {
    hipStream_t stream = nullptr;
    FitRecord rec;                            // of its last whole fit (a slice records into its slot instead)
    hipEvent_t ev_done = nullptr;             // end of this context's last call
    bool has_done = false;
    Inflight inflight;                        // its device-fit calls' caller buffers (fit_pipeline > 1)
    DevBuf diff;
    FitWs ws;
    bool fit_ctl = false;                     // rec.ctl_host holds (or will hold, in stream order) the kernel counters
    // host path (arima_fit_batch): device copies of one chunk and pinned staging of its input and outputs
    DevBuf d_series, d_coef, d_ll, d_status, d_neval, d_ngrad, d_flags, d_uinit;
    FitOut dev_out() const {
        return {d_coef.as<double>(), d_ll.as<double>(), d_status.as<int32_t>(), d_neval.as<int32_t>(),
                d_ngrad.as<int32_t>(), d_flags.as<uint8_t>()};
    }
    void *pin = nullptr;
    size_t pin_bytes = 0;
    int64_t chunk_first = -1, chunk_n = 0;    // the chunk whose results wait in `pin`
};

}  // namespace

struct arima_handle {
    int device = 0;
    int num_cus = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[kNumEvents] = {};
    hipEvent_t ev_done = nullptr;     // end of the last non-fit call's device work
    bool has_done = false;
    mutable std::mutex mu;
    std::string err;
    arima_fit_stats stats{};
    int smear = 1;           // Breeze 0.12 overlap semantics at ARIMA.scala:526: element-wise copy
    int grid_blocks_override = 0;
    int express_blocks = -1;       // k_cg_fit express workgroups (-1: num_cus / 16)
    int express_ring = 0;          // express hand-offs per launch (0: the whole ring, sts::kExpressRingEntries)
    int merge_live = sts::kMergeLiveDefault;    // k_cg_fit drain merge: hand over at <= this many live slots (0: off)
    // express CUs of the order search's concurrent fits (-1: as "express_blocks"). 0 by default: with 16 lanes in
    // flight each fit's express workgroups held whole CUs for the fit's duration, mostly waiting (C5 262 144:
    // 14 728 series/s with them, 16 659 without; profiles/r04/g_merge)
    int search_express_blocks = 0;
    int donate_evals = 0;          // k_cg_fit: evaluations before a slot may go to an express wave (0: kernel default)
    int donate_evals_drained = 0;  // ... once the batch's work counter has run out (0: kernel default)
    int chain_overhead = 0;        // k_cg_fit's objective-pass width model, 1/16 chains per step (0: kernel default 6)
    // k_hr_init: 0 = a lane per series; > 0 = that many single-wave workgroups (grid-stride); -1 (default) = 1 024
    // for pipelined device fits (fit_pipeline > 1: C2 9.47-9.55 -> 9.68-9.75 M series/s, profiles/r04/m_hrgrid),
    // else 0 (alone it is 25.2 vs 26.9 ms at C2)
    int hr_grid = -1;
    int row_pad = 0;               // doubles (multiple of 16) added to the differenced rows' stride
    // css-bobyqa layout: 1 = a wave per series (state in LDS), 0 = a lane per series, -1 (default) = a wave per series
    // for autoFit's retries and for fits of <= kBobyqaWaveMaxN series, else a lane per series. Bit-identical; measured
    // on C2 series: 1 024 fits 0.20 (wave) vs 0.62 s (lane), 16 384 fits ~1.6 (8 x the 1 024-series wave time: 2 048
    // series resident) vs 0.96 s, 65 536 fits 3.56 vs 1.79 s, autoFit of 65 536 series 11.98 vs 35.0 s
    // (profiles/r05/q_wave, r_occ2, g_tmpl). An objective parallel in time over the row in LDS (css_pit_lds) was
    // slower in this kernel: autoFit 19.3 s, 1 024 fits 0.27 s (s_pit)
    int bobyqa_wave = -1;
    // 1: device fits of d <= 1 difference into the k_difference workspace as before round 6 instead of reading the
    // caller's rows (option "fuse_diff" 0; results are identical, tests compare the two)
    int fuse_mode = 1;             // option "fuse_diff": 0 never, 1 where it pays (sts::fuse_pays), 2 always
    int64_t last_express = 0;
    int64_t last_grid = 0;
    int search_lanes = 8;          // concurrent fits of the order search (2/4/8: 1269/1303/1408 series/s, profiles/r02/g_c5)
    // fit contexts in rotation for device fits (option "fit_pipeline"). Default 3: consecutive asynchronous calls
    // overlap (one call's tail with the next one's differencing, init and bulk passes) and calls that share buffers
    // stay ordered (order_after_overlapping_fits). On the box's 4 hardware queues at C2 1M x 1024, 5 consecutive
    // calls: 1 / 2 / 3 / 4 contexts 6.68 / 8.30 / 10.02 / 9.97 M series/s; one call alone 151 ms at 1, 162 ms at 3
    // (drained bulk waves leave instead of turning express) -- profiles/r05/k_defp
    int pipeline = 3;
    // (Cutting ONE call into slices over several contexts was measured on the box's 4 queues at C2 1M x 1024 and
    // removed: 1 / 2 / 3 / 4 slices 6.91 / 6.39 / 6.35 / 4.47 M series/s, every slice ends with its own slowest
    // series; profiles/r05/c_af2/default_cs*.json.)
    // host path (arima_fit_batch): chunks of host_chunk series over host_pipeline fit contexts, the last ones halved
    // (host_tail). C2 1M x 1024 from pageable memory, 8 hardware queues: 262144 x 3 contexts 3.86 M series/s,
    // 131072 x 6 4.47-4.65, 65536 x 6 3.65 (profiles/r06/g_e2e); the upload runs at the link's 56 GB/s either way
    // (tools/h2d_bw.py, profiles/r06/d_ab/h2d.json), so the call is bound by the uploads plus its last fit's tail
    int host_pipeline = 3;         // contexts the chunked host path rotates over (option "host_pipeline"; arima_create)
    int64_t host_chunk = 1 << 18;  // series per chunk of the host path (option "host_chunk"; arima_create)
    int host_tail = 1;             // halve the last chunks (option "host_tail")
    // host path uploads: with host_copy_threads > 0 the caller's pageable rows are copied by that many threads into a
    // ring of pinned blocks, each block DMA'd while the threads fill the next (upload_staged); 0 (default) uploads
    // straight from pageable memory through the HIP runtime's own staging. Both reach the link's ~56 GB/s on the box
    // (tools/h2d_bw.py), and the runtime's staging measured slightly faster end to end (4.65 vs 4.47 M series/s at
    // C2, profiles/r06/g_e2e), so the staged ring stays an option for hosts whose pageable path is slower.
    int host_copy_threads = 0;
    static constexpr int kStageSlots = 3;
    static constexpr size_t kStageBytes = size_t(128) << 20;
    void *stage[kStageSlots] = {};
    hipEvent_t stage_ev[kStageSlots] = {};
    bool stage_used[kStageSlots] = {};
    unsigned stage_next = 0;
    int64_t fit_slice_bytes = 0;   // differenced workspace of one device-fit slice (option "fit_slice_bytes"; 0: from free HBM)
    SliceSlot slot[kSliceSlots];
    unsigned long long *slot_ctl = nullptr;     // pinned, kCtlWordsExt per slot
    unsigned slot_seq = 0;                      // slots taken so far
    unsigned slice_first = 0, slice_n = 0;      // slots of the last sliced fit call still pending (StatsFrom::kSlices)
    arima_fit_stats slice_acc{};                // ... and the stats of its slices whose slots were already reused
    DevBuf dev_fault;                           // sticky device record of the first fit-kernel fault (6 words)
    unsigned fit_seq = 0;          // fit calls so far (selects the context)
    // what arima_get_last_stats still has to complete: nothing (h->stats is final), the record of context stats_ctx,
    // the slots of a sliced fit, or the lanes' sums of an order search
    StatsFrom stats_from = StatsFrom::kNone;
    int stats_ctx = 0;
    arima_fit_stats host_acc{};    // host path: counters summed over its chunks
    FitCtx fctx[kMaxPipeline];
    // device workspaces of the building blocks
    DevBuf diff;
    DevBuf fc_ws;                  // the runtime-order forecast's per-series arrays (forecast_slices)
    // the staged arrays of the host-buffer entry points, one call's at a time (CallFrame::stage)
    DevBuf staging;
    // order search: the differenced series per d, the concurrent fit lanes
    DevBuf os_diff[kMaxD + 1];
    hipEvent_t ev_diff[kMaxD + 1] = {};
    SearchLane lanes[kMaxSearchLanes];
    // pinned: (kCtlWords + 1) words per lane of the last search, then (from lane kMaxSearchLanes's place on) the
    // lanes' kExtWords sums of the later words
    unsigned long long *search_acc_host = nullptr;
    // autoFit (arima_autofit_batch*): the differenced rows, the walk state, the rounds' per-order lists and results
    DevBuf af_rows, af_dsel, af_state, af_best, af_counts, af_lists, af_off, af_coef, af_ll, af_status, af_flags;
    DevBuf af_init, af_hrst, af_rlist, af_rcount;     // the round's inits and the css-bobyqa retry list
    int64_t *af_host = nullptr;                      // pinned: kAfCombosMax counts, kAfCombosMax row offsets, the retry count
    hipEvent_t ev_af = nullptr;
    int search_lanes_used = 0;
    int64_t search_n = 0, search_fits = 0;
    int64_t autofit_slice = 0;     // autoFit series per slice (option "autofit_slice"; 0 = from free HBM)
    // residual diagnostics (arima_residual_diagnostics_batch*): one slice of residuals
    int64_t diag_slice_bytes = 0;  // option "diag_slice_bytes"; 0 = 60 % of the free HBM, at least 1 GiB
    DevBuf dg_resid;
    // the design-matrix regressions (arima_arx_*, arima_bgtest_*, arima_bptest_*): one slice's designs, the tests' beta
    int64_t regress_slice_bytes = 0;   // option "regress_slice_bytes"; 0 = the rule of diag_slice_bytes
    DevBuf rg_ws, rg_beta;
    // the small models (EWMA, GARCH): the fit kernel's counters of the last fit
    DevBuf md_ctl;
    int64_t md_last_n = -1;        // series of the last EWMA / GARCH / ARGARCH fit (-1: none yet)
    DevBuf md_ar;                  // ARGARCH's AR stage per series: (c, phi), its CSS log-likelihood, its status
};

namespace {

int set_err(arima_handle *h, int code, const char *msg) {
    if (h) h->err = msg ? msg : "";
    return code;
}

#define HIPCHK(h, expr)                                                                                    \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) return set_err((h), ARIMA_E_DEVICE, hipGetErrorString(e_));                  \
    } while (0)

#define RCCHK(h, expr, what)                                                                               \
    do {                                                                                                   \
        int rc_ = (expr);                                                                                  \
        if (rc_ != ARIMA_OK) return set_err((h), rc_, what);                                               \
    } while (0)

// expr has set the message itself
#define PASSCHK(expr)                                                                                      \
    do {                                                                                                   \
        int rc_ = (expr);                                                                                  \
        if (rc_ != ARIMA_OK) return rc_;                                                                   \
    } while (0)

using sts::plan::round_up;
// Leading dimension of a differenced-row workspace: 128-B aligned rows of n doubles plus the handle's row_pad
static int64_t row_stride(const arima_handle *h, int64_t n) { return round_up(std::max<int64_t>(n, 1), 16) + h->row_pad; }

// uniform-per-call status fill (unsupported method, zero parameters, shape errors)
__global__ void k_fill_status(int64_t N, int k, const int32_t *__restrict__ prior, int32_t code,
                              double *__restrict__ coef_out, double *__restrict__ ll_out,
                              int32_t *__restrict__ status_out, int32_t *__restrict__ n_eval_out,
                              int32_t *__restrict__ n_grad_out, uint8_t *__restrict__ flags_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int st = code;
    if (prior && prior[i] != ARIMA_ST_OK) st = prior[i];
    for (int j = 0; j < k; ++j) coef_out[i * k + j] = __builtin_nan("");
    ll_out[i] = __builtin_nan("");
    status_out[i] = st;
    if (n_eval_out) n_eval_out[i] = 0;
    if (n_grad_out) n_grad_out[i] = 0;
    if (flags_out) flags_out[i] = 0;
}

// Take (read and clear) the sticky fault record rec[0..5] into rec[8..13] with atomic exchanges: a fault that a
// concurrent k_fault_merge records after the exchange of rec[0] stays for the next take instead of being cleared
// unseen (a plain read followed by a memset could lose it).
__global__ void k_fault_take(unsigned long long *__restrict__ rec) {
    if (threadIdx.x != 0) return;
    const unsigned long long code = atomicExch(&rec[0], 0ull);
    rec[8] = code;
    for (int i = 1; i < 6; ++i) rec[8 + i] = code ? atomicExch(&rec[i], 0ull) : 0ull;
}

// One grid point's fit into its search lane's counter sums (order-search stats, arima_get_last_stats): every kernel
// counter word and the fit's algorithmic flops (fit_stats.hpp search_acc_fit, which leaves the Hannan-Rissanen term
// out for AR-only fits; a fit's own stats count it there, fit_stats).
__global__ void k_search_acc(const unsigned long long *__restrict__ ctl, unsigned long long *__restrict__ acc,
                             int64_t N, int n, int p, int q, int I, int cg) {
    if (threadIdx.x == 0) {
        search_acc_fit(ctl, acc, N, n, p, q, I, cg);
        search_acc_ext(ctl, acc + kCtlWords + 1);
    }
}

// the first watchdog fault of a fit kernel (its fault words) into the handle's sticky device record
__global__ void k_fault_merge(const unsigned long long *__restrict__ ctl, unsigned long long *__restrict__ rec) {
    if (threadIdx.x != 0 || ctl[kCtlFault] == 0) return;
    if (atomicCAS(&rec[0], 0ull, ctl[kCtlFault]) == 0ull)
        for (int i = 1; i < kFaultWords; ++i) rec[i] = ctl[kCtlFault + i];
}

// what the KPSS test reports for every row of length T before it looks at one (kpsstest on no or one observation)
int32_t kpss_shape_status(int32_t T) {
    return T <= 0 ? ARIMA_ST_NO_DATA : (T < 2 ? ARIMA_ST_NOT_ENOUGH_DATA : ARIMA_ST_OK);
}

// p, q <= 5: the order-specialised kernels; 5 < p, q <= kGenMaxOrder (20): the runtime-order path (arima_generic.hip)
int check_orders(arima_handle *h, int p, int d, int q, int I) {
    if (p < 0 || q < 0 || d < 0 || (I != 0 && I != 1)) return set_err(h, ARIMA_E_INVALID_ARG, "bad order");
    if (!sts::gen_orders_ok(p, q)) return set_err(h, ARIMA_E_UNSUPPORTED, "p, q <= 20");
    if (d > 16) return set_err(h, ARIMA_E_UNSUPPORTED, "d <= 16");
    return ARIMA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Ordering. A non-fit call waits (on the device, not the host) for every earlier call: the building blocks share
// the handle's workspaces, and any call may read an earlier call's outputs. A fit call waits for the earlier
// non-fit calls (e.g. the sampler that wrote its input), for the previous call on its own context and, with
// fit_pipeline > 1 (default 3), for any in-flight fit whose buffers its own overlap (order_after_overlapping_fits);
// with fit_pipeline = 1 the previous call on its context is the previous fit, so calls run in issue order.
void begin_call(arima_handle *h, hipStream_t s) {
    if (h->has_done) hipStreamWaitEvent(s, h->ev_done, 0);
    for (auto &c : h->fctx)
        if (c.has_done) hipStreamWaitEvent(s, c.ev_done, 0);
}

hipError_t end_call(arima_handle *h, hipStream_t s) {
    hipError_t e = hipEventRecord(h->ev_done, s);
    if (e == hipSuccess) h->has_done = true;
    return e;
}

using sts::plan::Buf;
using sts::plan::buf_in;
using sts::plan::buf_opt_out;
using sts::plan::buf_out;
using sts::plan::strided_bytes;

enum CallFlavour { kDeviceBuffers, kHostBuffers };

// The frame of every non-fit entry point. It holds the handle's lock from construction; the argument checks run under
// it and touch no device. begin() selects the handle's device, picks the stream and orders it behind every earlier
// call. From then on every way out -- finish(), or an error return from the middle of the body -- records the call's
// end event, so later calls wait for whatever this one enqueued, and a host-buffer call also waits for its stream, so
// no copy into the caller's arrays is in flight when it returns. The first error keeps its code and message.
//
// The frame also holds the call's buffer table (sts::plan::Buf, one row per pointer argument), written down once by
// bind(). Both flavours of an entry point share one body: for device buffers dev<T>(i) is the caller's own pointer,
// for host buffers it is row i's copy in the handle's staging block, which begin() lays out (sts::plan::arena_layout)
// and uploads and finish() downloads. A null buffer that may be null takes no bytes and stays null for the kernels.
class CallFrame {
  public:
    CallFrame(arima_handle *h, CallFlavour flavour) : h_(h), lk_(h->mu), host_(flavour == kHostBuffers) {}
    CallFrame(const CallFrame &) = delete;
    CallFrame &operator=(const CallFrame &) = delete;
    ~CallFrame() { close(nullptr); }

    // The call's buffers; refuses a null one that is needed.
    int bind(std::initializer_list<Buf> table) {
        set(table);
        if (sts::plan::missing_buffer(buf_, n_)) return set_err(h_, ARIMA_E_INVALID_ARG, "null buffer");
        return ARIMA_OK;
    }
    // The rule of every entry point that checks its buffers (sts::plan::find_overlap), with its two messages
    int overlap() {
        switch (sts::plan::table_overlap(buf_, n_)) {
        case sts::plan::kOutputMeetsInput: return set_err(h_, ARIMA_E_INVALID_ARG, "an output overlaps an input");
        case sts::plan::kOutputsMeet: return set_err(h_, ARIMA_E_INVALID_ARG, "outputs overlap");
        default: return ARIMA_OK;
        }
    }

    int begin(void *stream = nullptr) {
        HIPCHK(h_, hipSetDevice(h_->device));
        s_ = stream ? (hipStream_t)stream : h_->stream;
        begin_call(h_, s_);
        open_ = true;
        return host_ && n_ ? upload() : ARIMA_OK;
    }
    hipStream_t s() const { return s_; }

    // The building blocks, which check no buffer: their table after begin() (and after their padded upload). A null
    // buffer reaches the copy, which refuses it.
    int stage(std::initializer_list<Buf> table) {
        set(table);
        return upload();
    }
    template <class T>
    T *dev(int i) const {
        const bool staged = host_ && (buf_[i].p || buf_[i].need);
        return static_cast<T *>(staged ? h_->staging.as<char>() + off_[i] : const_cast<void *>(buf_[i].p));
    }
    int64_t bytes(int i) const { return buf_[i].bytes; }

    // staged row i to a host array of the caller's that is not the row's own (the ARIMA effects pair)
    int download(int i, void *dst) {
        HIPCHK(h_, hipMemcpyAsync(dst, dev<char>(i), (size_t)buf_[i].bytes, hipMemcpyDeviceToHost, s_));
        return ARIMA_OK;
    }

    // The way out of a body that got this far: after rc == ARIMA_OK the staged outputs go back to the host; then the
    // end event and, for host buffers, the wait. Returns the first error.
    int finish(int rc = ARIMA_OK) {
        for (int i = 0; host_ && i < n_ && rc == ARIMA_OK; ++i) {
            if (!buf_[i].written() || !buf_[i].bytes) continue;
            const hipError_t e = hipMemcpyAsync(const_cast<void *>(buf_[i].p), dev<char>(i), (size_t)buf_[i].bytes,
                                                hipMemcpyDeviceToHost, s_);
            if (e != hipSuccess) rc = set_err(h_, ARIMA_E_DEVICE, hipGetErrorString(e));
        }
        close(&rc);
        return rc;
    }

  private:
    void set(std::initializer_list<Buf> table) {
        assert(table.size() <= (size_t)sts::plan::kMaxBufs);
        n_ = 0;
        for (const Buf &b : table) {
            buf_[n_] = b;
            if ((!b.p && !b.need) || b.bytes < 0) buf_[n_].bytes = 0;
            ++n_;
        }
    }
    // grows the staging block once for the whole table and uploads what the call reads
    int upload() {
        size_t bytes[sts::plan::kMaxBufs];
        for (int i = 0; i < n_; ++i) bytes[i] = (size_t)buf_[i].bytes;
        const size_t total = sts::plan::arena_layout(bytes, n_, off_);
        RCCHK(h_, h_->staging.ensure(std::max<size_t>(total, 256)), "staging");
        for (int i = 0; i < n_; ++i)
            if (buf_[i].read() && buf_[i].bytes)
                HIPCHK(h_, hipMemcpyAsync(h_->staging.as<char>() + off_[i], buf_[i].p, bytes[i], hipMemcpyHostToDevice,
                                          s_));
        return ARIMA_OK;
    }
    void close(int *rc) {
        if (!open_) return;
        open_ = false;
        hipError_t e = end_call(h_, s_);
        if (host_) {
            const hipError_t w = hipStreamSynchronize(s_);
            if (e == hipSuccess) e = w;
        }
        if (e != hipSuccess && rc && *rc == ARIMA_OK) *rc = set_err(h_, ARIMA_E_DEVICE, hipGetErrorString(e));
    }
    arima_handle *h_;
    std::lock_guard<std::mutex> lk_;
    const bool host_;
    hipStream_t s_ = nullptr;
    bool open_ = false;
    int n_ = 0;
    Buf buf_[sts::plan::kMaxBufs];
    size_t off_[sts::plan::kMaxBufs];
};

// The workspace forecasts (k_gen_forecast, k_arimax_gen_forecast) over N series of w workspace doubles each: slices of
// at most 2^27 doubles (1 GiB) of h->fc_ws, at least one series; launch(f, m, ws) runs series [f, f + m) on the stream
// of the call, where a slice's kernel ends before the next one's starts
template <class Launch>
int forecast_slices(arima_handle *h, int64_t N, int64_t w, const char *what, Launch launch) {
    const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(N, (int64_t(1) << 27) / std::max<int64_t>(w, 1)));
    RCCHK(h, h->fc_ws.ensure((size_t)std::min(chunk, N) * w * sizeof(double)), "forecast workspace");
    for (int64_t f = 0; f < N; f += chunk) RCCHK(h, launch(f, std::min(chunk, N - f), h->fc_ws.as<double>()), what);
    return ARIMA_OK;
}

}  // namespace

namespace sts {
int hr_shape_status_host(int n, int p, int q, int I);
}

extern "C" {

int arima_num_params(int p, int q, int include_intercept) { return p + q + (include_intercept ? 1 : 0); }

const char *arima_status_name(int s) {
    switch (s) {
    case ARIMA_ST_OK: return "OK";
    case ARIMA_ST_MAX_EVAL: return "MAX_EVAL";
    case ARIMA_ST_BRACKET_MAX_EVAL: return "BRACKET_MAX_EVAL";
    case ARIMA_ST_MAX_ITER: return "MAX_ITER";
    case ARIMA_ST_SINGULAR: return "SINGULAR";
    case ARIMA_ST_NOT_ENOUGH_DATA: return "NOT_ENOUGH_DATA";
    case ARIMA_ST_NO_DATA: return "NO_DATA";
    case ARIMA_ST_BAD_INTERVAL: return "BAD_INTERVAL";
    case ARIMA_ST_ZERO_PARAMS: return "ZERO_PARAMS";
    case ARIMA_ST_UNSUPPORTED_METHOD: return "UNSUPPORTED_METHOD";
    case ARIMA_ST_SERIES_TOO_SHORT: return "SERIES_TOO_SHORT";
    case ARIMA_ST_NOT_STATIONARY: return "NOT_STATIONARY";
    case ARIMA_ST_NO_MODEL: return "NO_MODEL";
    case ARIMA_ST_TOO_FEW_PARAMS: return "TOO_FEW_PARAMS";
    default: return "UNKNOWN";
    }
}

int arima_create(int device, arima_handle **out) {
    if (!out) return ARIMA_E_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return ARIMA_E_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return ARIMA_E_DEVICE;
    arima_handle *h = new arima_handle();
    h->device = device;
    // the host path's contexts need hardware queues of their own (HIP maps a process's streams onto
    // GPU_MAX_HW_QUEUES of them, default 4): 6 contexts of 131072-series chunks with 8 or more queues, else 3 of 262144
    // (profiles/r06/e_split, g_e2e: on 4 queues 4+ contexts serialise and run slower than 3)
    if (const char *q = getenv("GPU_MAX_HW_QUEUES")) {
        if (atoi(q) >= 8) {
            h->host_pipeline = 6;
            h->host_chunk = 1 << 17;
        }
    }
    hipDeviceGetAttribute(&h->num_cus, hipDeviceAttributeMultiprocessorCount, device);
    int rc = ARIMA_OK;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) rc = ARIMA_E_DEVICE;
    for (auto &e : h->ev)
        if (rc == ARIMA_OK && hipEventCreate(&e) != hipSuccess) rc = ARIMA_E_DEVICE;
    if (rc == ARIMA_OK && hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming) != hipSuccess) rc = ARIMA_E_DEVICE;
    for (auto &c : h->fctx) {
        if (rc == ARIMA_OK && hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking) != hipSuccess) rc = ARIMA_E_DEVICE;
        if (rc == ARIMA_OK) rc = c.rec.create();
        if (rc == ARIMA_OK && hipEventCreateWithFlags(&c.ev_done, hipEventDisableTiming) != hipSuccess) rc = ARIMA_E_DEVICE;
        if (rc == ARIMA_OK && hipHostMalloc((void **)&c.rec.ctl_host, kCtlWordsExt * sizeof(unsigned long long), 0) != hipSuccess)
            rc = ARIMA_E_OOM;
    }
    if (rc == ARIMA_OK &&
        hipHostMalloc((void **)&h->slot_ctl, (size_t)kSliceSlots * kCtlWordsExt * sizeof(unsigned long long), 0) != hipSuccess)
        rc = ARIMA_E_OOM;
    for (int j = 0; j < kSliceSlots && rc == ARIMA_OK; ++j) h->slot[j].rec.ctl_host = h->slot_ctl + (size_t)j * kCtlWordsExt;
    if (rc == ARIMA_OK && hipHostMalloc((void **)&h->search_acc_host,
                                        (size_t)kMaxSearchLanes * (kCtlWords + 1 + kExtWords) * sizeof(unsigned long long), 0) != hipSuccess)
        rc = ARIMA_E_OOM;
    if (rc == ARIMA_OK && h->dev_fault.ensure(16 * sizeof(unsigned long long)) != ARIMA_OK) rc = ARIMA_E_OOM;
    if (rc == ARIMA_OK && hipMemset(h->dev_fault.ptr, 0, 16 * sizeof(unsigned long long)) != hipSuccess) rc = ARIMA_E_DEVICE;
    if (rc != ARIMA_OK) {
        arima_destroy(h);
        return rc;
    }
    *out = h;
    return ARIMA_OK;
}

int arima_destroy(arima_handle *h) {
    if (!h) return ARIMA_E_INVALID_ARG;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->has_done) hipEventSynchronize(h->ev_done);
    for (auto &l : h->lanes) {
        if (l.stream) {
            hipStreamSynchronize(l.stream);
            hipStreamDestroy(l.stream);
        }
        if (l.ev_fit) hipEventDestroy(l.ev_fit);
        if (l.ev_sel) hipEventDestroy(l.ev_sel);
    }
    for (auto &c : h->fctx) {
        if (c.stream) {
            hipStreamSynchronize(c.stream);
            hipStreamDestroy(c.stream);
        }
        c.rec.destroy();
        if (c.ev_done) hipEventDestroy(c.ev_done);
        for (auto &e : c.inflight.ev)
            if (e) hipEventDestroy(e);
        if (c.rec.ctl_host) hipHostFree(c.rec.ctl_host);
        if (c.pin) hipHostFree(c.pin);
    }
    for (auto &e : h->ev_diff)
        if (e) hipEventDestroy(e);
    for (auto &sl : h->slot) sl.rec.destroy();
    for (int j = 0; j < arima_handle::kStageSlots; ++j) {
        if (h->stage_ev[j]) {
            hipEventSynchronize(h->stage_ev[j]);
            hipEventDestroy(h->stage_ev[j]);
        }
        if (h->stage[j]) hipHostFree(h->stage[j]);
    }
    if (h->slot_ctl) hipHostFree(h->slot_ctl);
    if (h->search_acc_host) hipHostFree(h->search_acc_host);
    if (h->af_host) hipHostFree(h->af_host);
    if (h->ev_af) hipEventDestroy(h->ev_af);
    for (auto &e : h->ev)
        if (e) hipEventDestroy(e);
    if (h->ev_done) hipEventDestroy(h->ev_done);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;                                  // every DevBuf workspace frees itself
    return ARIMA_OK;
}

const char *arima_last_error(const arima_handle *h) { return h ? h->err.c_str() : "null handle"; }

// Completes h->stats from where the last call left them (StatsFrom): the sources are consumed, a second call
// returns the same values.
int arima_get_last_stats(const arima_handle *hc, arima_fit_stats *out) {
    if (!hc || !out) return ARIMA_E_INVALID_ARG;
    arima_handle *h = const_cast<arima_handle *>(hc);   // the lazy completion below only fills h->stats
    std::lock_guard<std::mutex> lk(h->mu);
    hipError_t e = hipSuccess;
    if (h->stats_from == StatsFrom::kContext && h->fctx[h->stats_ctx].rec.ps.valid) {
        FitCtx &c = h->fctx[h->stats_ctx];
        hipSetDevice(h->device);
        if ((e = hipEventSynchronize(c.ev_done)) == hipSuccess) h->stats = c.rec.stats();
        if (e == hipSuccess) c.rec.ps.valid = false;
    } else if (h->stats_from == StatsFrom::kSlices && h->slice_n > 0) {   // a sliced fit: the sum over its slices
        hipSetDevice(h->device);
        arima_fit_stats acc = h->slice_acc;
        for (unsigned j = 0; j < h->slice_n && e == hipSuccess; ++j) {
            const FitRecord &r = h->slot[(h->slice_first + j) % kSliceSlots].rec;
            if ((e = hipEventSynchronize(r.ev[4])) == hipSuccess) acc_stats(acc, r.stats());
        }
        if (e == hipSuccess) {
            h->stats = acc;
            h->slice_n = 0;
            h->slice_acc = arima_fit_stats{};
        }
    } else if (h->stats_from == StatsFrom::kSearch && h->search_lanes_used > 0) {   // the sums over a search's fits
        hipSetDevice(h->device);
        if ((e = hipEventSynchronize(h->ev[4])) == hipSuccess) {
            float ms = 0;
            hipEventElapsedTime(&ms, h->ev[0], h->ev[3]);
            h->stats = search_stats(h->search_acc_host, h->search_lanes_used, h->search_n * h->search_fits,
                                    h->last_grid, h->last_express, ms);
            search_stats_ext(h->stats, h->search_acc_host + (size_t)kMaxSearchLanes * (kCtlWords + 1), h->search_lanes_used);
            h->search_lanes_used = 0;
        }
    }
    if (e != hipSuccess) return set_err(h, ARIMA_E_DEVICE, "stats: device error");
    *out = h->stats;
    return ARIMA_OK;
}

// the message of a fit kernel's watchdog fault record (its six fault words)
static int report_fault(arima_handle *h, const unsigned long long *f) {
    char msg[160];
    snprintf(msg, sizeof msg, "fit kernel watchdog fault %llu (info %llu %llu %llu %llu %llu)", f[0], f[1], f[2], f[3],
             f[4], f[5]);
    return set_err(h, ARIMA_E_DEVICE, msg);
}

// A finished fit kernel of context c recorded a watchdog fault (k_cg_fit's hand-off): its results are incomplete.
static int check_fault(arima_handle *h, FitCtx &c) {
    if (!c.fit_ctl || c.rec.ctl_host[kCtlFault] == 0) return ARIMA_OK;
    c.fit_ctl = false;                      // reported once
    return report_fault(h, c.rec.ctl_host + kCtlFault);
}

static int take_fault(arima_handle *h);

int arima_synchronize(arima_handle *h) {
    if (!h) return ARIMA_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    if (h->has_done) HIPCHK(h, hipEventSynchronize(h->ev_done));
    int rc = ARIMA_OK;
    for (auto &c : h->fctx) {
        if (c.has_done) HIPCHK(h, hipEventSynchronize(c.ev_done));
        if (rc == ARIMA_OK) rc = check_fault(h, c);
    }
    for (auto &l : h->lanes)
        if (l.stream) HIPCHK(h, hipStreamSynchronize(l.stream));
    // the sticky record every fit kernel's counters are merged into (sliced fits, order-search lanes, contexts whose
    // pinned counters a later call has already overwritten)
    const int rf = take_fault(h);
    if (rc == ARIMA_OK) rc = rf;
    return rc;
}

int arima_set_option(arima_handle *h, const char *name, int64_t value) {
    if (!h || !name) return ARIMA_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!strcmp(name, "smear")) { h->smear = value ? 1 : 0; return ARIMA_OK; }
    if (!strcmp(name, "bobyqa_wave")) { h->bobyqa_wave = value < 0 ? -1 : (value ? 1 : 0); return ARIMA_OK; }
    if (!strcmp(name, "fuse_diff")) { h->fuse_mode = (int)std::min<int64_t>(2, std::max<int64_t>(0, value)); return ARIMA_OK; }
    if (!strcmp(name, "chain_overhead")) { h->chain_overhead = (int)std::min<int64_t>(4096, std::max<int64_t>(0, value)); return ARIMA_OK; }
    if (!strcmp(name, "autofit_slice")) { h->autofit_slice = std::max<int64_t>(0, value); return ARIMA_OK; }
    if (!strcmp(name, "row_pad")) {                 // doubles, rounded up to whole 128-B lines
        h->row_pad = (int)round_up(std::min<int64_t>(4096, std::max<int64_t>(0, value)), 16);
        return ARIMA_OK;
    }
    if (!strcmp(name, "hr_grid")) { h->hr_grid = (int)std::min<int64_t>(1 << 20, std::max<int64_t>(-1, value)); return ARIMA_OK; }
    if (!strcmp(name, "express_ring")) {
        h->express_ring = (int)std::min<int64_t>(sts::kExpressRingEntries, std::max<int64_t>(0, value));
        return ARIMA_OK;
    }
    if (!strcmp(name, "search_express_blocks")) {
        h->search_express_blocks = (int)std::max<int64_t>(-1, value);
        return ARIMA_OK;
    }
    if (!strcmp(name, "donate_evals")) { h->donate_evals = (int)std::max<int64_t>(0, value); return ARIMA_OK; }
    if (!strcmp(name, "donate_evals_drained")) {
        h->donate_evals_drained = (int)std::max<int64_t>(0, value);
        return ARIMA_OK;
    }
    if (!strcmp(name, "merge_live")) { h->merge_live = (int)std::min<int64_t>(64, std::max<int64_t>(0, value)); return ARIMA_OK; }
    if (!strcmp(name, "express_blocks")) { h->express_blocks = (int)std::max<int64_t>(-1, value); return ARIMA_OK; }
    if (!strcmp(name, "grid_blocks")) { h->grid_blocks_override = (int)std::max<int64_t>(0, value); return ARIMA_OK; }
    if (!strcmp(name, "search_lanes")) {
        h->search_lanes = (int)std::min<int64_t>(kMaxSearchLanes, std::max<int64_t>(1, value));
        return ARIMA_OK;
    }
    if (!strcmp(name, "fit_pipeline")) {
        h->pipeline = (int)std::min<int64_t>(kMaxPipeline, std::max<int64_t>(1, value));
        return ARIMA_OK;
    }
    if (!strcmp(name, "host_pipeline")) {
        h->host_pipeline = (int)std::min<int64_t>(kMaxPipeline, std::max<int64_t>(1, value));
        return ARIMA_OK;
    }
    if (!strcmp(name, "host_chunk")) { h->host_chunk = std::max<int64_t>(1, value); return ARIMA_OK; }
    if (!strcmp(name, "host_tail")) { h->host_tail = value ? 1 : 0; return ARIMA_OK; }
    if (!strcmp(name, "host_copy_threads")) {
        h->host_copy_threads = (int)std::min<int64_t>(64, std::max<int64_t>(0, value));
        return ARIMA_OK;
    }
    if (!strcmp(name, "fit_slice_bytes")) { h->fit_slice_bytes = std::max<int64_t>(0, value); return ARIMA_OK; }
    if (!strcmp(name, "diag_slice_bytes")) { h->diag_slice_bytes = std::max<int64_t>(0, value); return ARIMA_OK; }
    if (!strcmp(name, "regress_slice_bytes")) { h->regress_slice_bytes = std::max<int64_t>(0, value); return ARIMA_OK; }
    return set_err(h, ARIMA_E_INVALID_ARG, "unknown option");
}

int arima_get_option(const arima_handle *hc, const char *name, int64_t *value) {
    if (!hc || !name || !value) return ARIMA_E_INVALID_ARG;
    const arima_handle *h = hc;
    std::lock_guard<std::mutex> lk(h->mu);
    const struct { const char *n; int64_t v; } opts[] = {
        {"smear", h->smear}, {"express_blocks", h->express_blocks}, {"grid_blocks", h->grid_blocks_override},
        {"search_lanes", h->search_lanes}, {"fit_pipeline", h->pipeline}, {"host_pipeline", h->host_pipeline},
        {"host_chunk", h->host_chunk}, {"fit_slice_bytes", h->fit_slice_bytes}, {"express_ring", h->express_ring},
        {"hr_grid", h->hr_grid}, {"row_pad", h->row_pad}, {"bobyqa_wave", h->bobyqa_wave}, {"merge_live", h->merge_live},
        {"search_express_blocks", h->search_express_blocks}, {"donate_evals", h->donate_evals},
        {"donate_evals_drained", h->donate_evals_drained}, {"fuse_diff", h->fuse_mode}, {"autofit_slice", h->autofit_slice},
        {"host_copy_threads", h->host_copy_threads}, {"chain_overhead", h->chain_overhead}, {"host_tail", h->host_tail},
        {"diag_slice_bytes", h->diag_slice_bytes}, {"regress_slice_bytes", h->regress_slice_bytes}};
    for (const auto &o : opts)
        if (!strcmp(name, o.n)) {
            *value = o.v;
            return ARIMA_OK;
        }
    return ARIMA_E_INVALID_ARG;
}

// a fit call's part of the ordering rules (stated at begin_call)
static void begin_fit(arima_handle *h, FitCtx &c, hipStream_t s) {
    if (h->has_done) hipStreamWaitEvent(s, h->ev_done, 0);
    if (c.has_done) hipStreamWaitEvent(s, c.ev_done, 0);
}

// fit_pipeline > 1: consecutive fit calls run concurrently on different contexts, unless one reads what an in-flight
// call writes, writes what it reads, or writes the same memory -- then the new call waits for that call's end (so a
// caller may chain fits, e.g. one fit's coefficients as the next one's user inits, or reuse one output buffer,
// without synchronising: the same results as fit_pipeline 1)
static bool calls_meet(const CallSpans &x, const CallSpans &y) {
    for (int a = 0; a < 6; ++a) {
        for (int b = 0; b < 2; ++b)
            if (x.out[a].meets(y.in[b])) return true;
        for (int b = 0; b < 6; ++b)
            if (x.out[a].meets(y.out[b])) return true;
    }
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 6; ++b)
            if (x.in[a].meets(y.out[b])) return true;
    return false;
}

// Returns the event to record at the new call's end (nullptr once its context tracks kInflightMax calls).
static hipEvent_t order_after_overlapping_fits(arima_handle *h, int ci, const CallSpans &cs, hipStream_t s) {
    for (int j = 0; j < kMaxPipeline; ++j) {
        FitCtx &o = h->fctx[j];
        if (!o.has_done || hipEventQuery(o.ev_done) == hipSuccess) {   // everything issued there has finished
            o.inflight.n = 0;
            o.inflight.overflow = false;
            continue;
        }
        if (j == ci) continue;                     // begin_fit already orders the call after its context's last one
        if (o.inflight.overflow) {
            hipStreamWaitEvent(s, o.ev_done, 0);
            continue;
        }
        for (int e = 0; e < o.inflight.n; ++e)
            if (calls_meet(cs, o.inflight.call[e])) hipStreamWaitEvent(s, o.inflight.ev[e], 0);
    }
    Inflight &f = h->fctx[ci].inflight;
    if (f.n == kInflightMax) {
        f.overflow = true;
        return nullptr;
    }
    if (!f.ev[f.n] && hipEventCreateWithFlags(&f.ev[f.n], hipEventDisableTiming) != hipSuccess) {
        f.overflow = true;
        return nullptr;
    }
    f.call[f.n] = cs;
    return f.ev[f.n++];
}

static CallSpans call_spans(const double *series, int64_t N, int32_t T, int64_t ld, int k, const double *uinit,
                            const FitOut &o) {
    CallSpans cs;
    if (N <= 0) return cs;
    cs.in[0] = ByteSpan(series, ((N - 1) * ld + std::max<int64_t>(T, 0)) * (int64_t)sizeof(double));
    cs.in[1] = ByteSpan(uinit, N * k * (int64_t)sizeof(double));
    cs.out[0] = ByteSpan(o.coef, N * k * (int64_t)sizeof(double));
    cs.out[1] = ByteSpan(o.ll, N * (int64_t)sizeof(double));
    cs.out[2] = ByteSpan(o.status, N * (int64_t)sizeof(int32_t));
    cs.out[3] = ByteSpan(o.n_eval, N * (int64_t)sizeof(int32_t));
    cs.out[4] = ByteSpan(o.n_grad, N * (int64_t)sizeof(int32_t));
    cs.out[5] = ByteSpan(o.flags, N);
    return cs;
}

static hipError_t end_fit(FitCtx &c, hipStream_t s) {
    hipError_t e = hipEventRecord(c.ev_done, s);
    if (e == hipSuccess) c.has_done = true;
    return e;
}

struct FitOpts {                   // how fit_kernels runs its fit
    // other fits run concurrently (the order search's lanes, pipelined calls), so the fit kernel's drained workgroups
    // exit instead of joining its express pool
    bool shared_gpu = false;
    int express_cus = -2;          // the fit kernel's express CUs; -2 = the "express_blocks" option (the search passes its own)
    bool search = false;           // a lane of the order search: k_hr_init keeps a lane per series
    // 1: y holds the caller's RAW rows (leading dimension ldn) of a d = 1 fit, differenced inside every pass (fused
    // differencing, arima_device.hpp stream_row); 0: y holds differenced rows
    int dd = 0;
    hipEvent_t ev_mid = nullptr;   // recorded between the init and the fit kernel
};

// Hannan-Rissanen init (unless user init) and the fit kernel -- or the AR-only shortcut, or a uniform per-series
// status -- over already-differenced rows y (N x n, leading dimension ldn), on stream s with workspace ws.
static int fit_kernels(arima_handle *h, FitWs &ws, const double *y, int64_t ldn, int n, int64_t N, int32_t p,
                       int32_t q, int32_t I, int32_t method, const double *d_user_init, const FitOut &o, hipStream_t s,
                       int64_t *grid_out, int64_t *express_out, const FitOpts &opt = FitOpts{}) {
    const int k = I + p + q;
    const int dd = opt.dd;
    *grid_out = 0;
    *express_out = 0;
    RCCHK(h, ws.reserve(N, k), "workspace");
    // the fit kernel's counters and express-ring ready words, initialised by the kernel that runs before it
    // (k_hr_init, or one k_fit_prep dispatch) instead of up to six fill dispatches (round 6)
    sts::FitPrep prep;
    prep.ctl = ws.ctl.as<unsigned long long>();
    prep.xready = ws.xready.as<unsigned>();
    prep.xready_words = sts::kExpressReadyBytes / 4;
    prep.v19 = (unsigned long long)std::max(h->express_ring, 0);
    prep.v44 = (unsigned long long)std::max(h->merge_live, 0);
    prep.v45 = (unsigned long long)std::max(h->donate_evals, 0);
    prep.v46 = (unsigned long long)std::max(h->donate_evals_drained, 0);
    prep.v47 = (unsigned long long)std::max(h->chain_overhead, 0);
    const bool cg = !(p > 0 && q == 0) && method == ARIMA_METHOD_CSS_CGD && k > 0;
    const bool gen = sts::gen_order(p, q);                     // above the compiled orders: arima_generic.hip
    if (!cg || gen) prep.xready_words = 0;                     // no express ring: only the counters are read
    if (p > 0 && q == 0) {                                     // AR-only shortcut, method never checked
        RCCHK(h, sts::launch_fit_prep(prep, s), "fit_prep");
        if (opt.ev_mid) HIPCHK(h, hipEventRecord(opt.ev_mid, s));
        if (gen) RCCHK(h, sts::launch_gen_ar_fit(y, ldn, n, N, p, I, o, dd, s), "ar_fit");
        else RCCHK(h, sts::launch_ar_fit(y, ldn, n, N, p, I, o, s, dd), "ar_fit");
        return ARIMA_OK;
    }
    const double *init = d_user_init;
    const int32_t *init_status = nullptr;
    if (!d_user_init) {
        if (gen)
            RCCHK(h, sts::launch_gen_hr_init(y, ldn, n, N, p, q, I, ws.init.as<double>(), ws.hr_status.as<int32_t>(),
                                             dd, prep, s), "hr_init");
        else
            RCCHK(h, sts::launch_hr_init(y, ldn, n, N, p, q, I, ws.init.as<double>(), ws.hr_status.as<int32_t>(), s,
                                         h->hr_grid >= 0 ? h->hr_grid : (opt.shared_gpu && !opt.search ? 1024 : 0), dd,
                                         prep), "hr_init");
        init = ws.init.as<double>();
        init_status = ws.hr_status.as<int32_t>();
    } else {
        RCCHK(h, sts::launch_fit_prep(prep, s), "fit_prep");
    }
    if (opt.ev_mid) HIPCHK(h, hipEventRecord(opt.ev_mid, s));
    if (method == ARIMA_METHOD_CSS_BOBYQA && k > 0) {           // fitWithCSSBOBYQA, ARIMA.scala:106, :130-160
        RCCHK(h, sts::launch_bobyqa_fit(y, ldn, n, N, p, q, I, init, init_status, nullptr, o,
                                        h->bobyqa_wave < 0 ? N <= kBobyqaWaveMaxN : h->bobyqa_wave != 0, s),
              "bobyqa_fit");
        return ARIMA_OK;
    }
    if (method != ARIMA_METHOD_CSS_CGD || k == 0) {
        const unsigned grid = (unsigned)((N + 255) / 256);
        const int32_t code = (method != ARIMA_METHOD_CSS_CGD) ? ARIMA_ST_UNSUPPORTED_METHOD : ARIMA_ST_ZERO_PARAMS;
        hipLaunchKernelGGL(k_fill_status, dim3(grid), dim3(256), 0, s, N, k, init_status, code, o.coef, o.ll, o.status,
                           o.n_eval, o.n_grad, o.flags);
        HIPCHK(h, hipGetLastError());
        return ARIMA_OK;
    }
    if (gen) {                                                  // fitWithCSSCGD at runtime orders, a lane per series
        RCCHK(h, sts::launch_gen_fit(y, ldn, n, N, p, q, I, h->smear, init, init_status, o,
                                     ws.ctl.as<unsigned long long>(), dd, s), "gen_fit");
        return ARIMA_OK;
    }
    // one persistent workgroup per CU (4 waves x the kernel's optimizer slots), the last num_cus/16 of them express
    // workgroups (k_cg_fit's long-series path); fewer bulk blocks when the batch cannot fill them
    // (express_blocks and grid_blocks count CUs' worth of workgroups: x kFitBlocksPerCU single-wave workgroups)
    const int cus = std::max(1, h->num_cus);
    const int xopt = opt.express_cus >= -1 ? opt.express_cus : h->express_blocks;
    int xcus = xopt >= 0 ? xopt : std::max(1, cus / 16);
    if (xcus >= cus) xcus = cus - 1;
    int bcus = h->grid_blocks_override;
    if (bcus <= 0) bcus = std::max(1, cus - xcus);
    const int bpc = sts::kFitBlocksPerCU;
    int xblocks = xcus * bpc;
    int blocks = bcus * bpc;
    const int per_block = std::max(1, sts::cg_fit_series_per_block(p, q, I));
    const int64_t need = (N + per_block - 1) / per_block;
    if (blocks > need) blocks = (int)need;
    *grid_out = blocks;
    *express_out = xcus;                    // in CUs, the unit of the "express_blocks" option
    RCCHK(h, sts::launch_cg_fit(y, ldn, n, N, p, q, I, h->smear, init, init_status, o, ws.ctl.as<unsigned long long>(),
                                blocks, xblocks, ws.xring.as<unsigned char>(), ws.xready.as<unsigned>(),
                                opt.shared_gpu ? 0 : 1, s, dd), "cg_fit");
    hipLaunchKernelGGL(k_fault_merge, dim3(1), dim3(64), 0, s, ws.ctl.as<unsigned long long>(),
                       h->dev_fault.as<unsigned long long>());
    HIPCHK(h, hipGetLastError());
    return ARIMA_OK;
}

// Grow the workspaces of the first `count` contexts to an N x ldn batch with k parameters at once, so that no
// workspace grows (hipFree synchronises the device) while fits of other contexts are in flight.
static int reserve_fit_ws(arima_handle *h, int count, int64_t N, int64_t ldn, int k, bool diff_ws = true) {
    for (int j = 0; j < count; ++j) {
        FitCtx &c = h->fctx[j];
        if (diff_ws) RCCHK(h, c.diff.ensure((size_t)N * ldn * sizeof(double)), "workspace");
        RCCHK(h, c.ws.reserve(N, k), "workspace");
    }
    return ARIMA_OK;
}

// One fit on context c, enqueued on stream s: the caller has checked the arguments, selected the device and ordered s
// after what the fit depends on. Its timing events and counter copy go to rec: the context's own record, or the slot
// record of one slice of a sliced call (the context then keeps no pending stats of its own).
// shared_gpu: fits of other contexts may run concurrently, so the fit kernel's drained workgroups exit (making room
// for the next fit) instead of joining its express pool.
static int fit_device_locked(arima_handle *h, FitCtx &c, FitRecord &rec, int reserve, const double *d_series, int64_t N,
                             int32_t T, int64_t ld, int32_t p, int32_t d, int32_t q, int32_t I, int32_t method,
                             const double *d_user_init, const FitOut &o, hipStream_t s, bool shared_gpu) {
    const int k = I + p + q;
    const int n = std::max(T - d, 0);
    c.rec.ps = rec.ps = FitShape{};
    if (N == 0) return ARIMA_OK;
    // Fused differencing (round 6): css-cgd fits (and the AR-only shortcut) of d <= 1 read the caller's rows directly
    // -- d = 0 as they are, d = 1 differenced inside every pass (arima_device.hpp stream_row) -- instead of a
    // differenced copy written by k_difference (17 GB of HBM traffic per 1M x 1024 fit, a pipeline stage of its own,
    // and an N x T workspace per fit context). d >= 2 and css-bobyqa keep the copy.
    const bool fused = d <= 1 && (method == ARIMA_METHOD_CSS_CGD || (p > 0 && q == 0)) &&
                       (h->fuse_mode == 2 || (h->fuse_mode == 1 && sts::fuse_pays(p, q)));
    const int64_t ldn = fused ? ld : row_stride(h, n);
    const double *rows = fused ? d_series : nullptr;
    RCCHK(h, reserve_fit_ws(h, reserve, N, ldn, k, !fused), "workspace");
    HIPCHK(h, hipEventRecord(rec.ev[0], s));
    if (!fused) {
        RCCHK(h, sts::launch_difference(d_series, ld, c.diff.as<double>(), ldn, N, T, d, 1, s), "difference");
        rows = c.diff.as<double>();
    }
    HIPCHK(h, hipEventRecord(rec.ev[1], s));
    FitShape &ps = rec.ps;
    FitOpts opt;
    opt.shared_gpu = shared_gpu;
    opt.dd = fused ? d : 0;
    opt.ev_mid = rec.ev[2];
    RCCHK(h, fit_kernels(h, c.ws, rows, ldn, n, N, p, q, I, method, d_user_init, o, s, &ps.grid, &ps.express, opt),
          "fit");
    HIPCHK(h, hipEventRecord(rec.ev[3], s));
    h->last_grid = ps.grid;
    h->last_express = ps.express;
    HIPCHK(h, hipMemcpyAsync(rec.ctl_host, c.ws.ctl.ptr, kCtlWordsExt * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    c.fit_ctl = &rec == &c.rec;             // check_fault reads the context's own copy only
    ps.N = N;
    ps.n = n;
    ps.p = p;
    ps.q = q;
    ps.I = I;
    ps.ar_only = p > 0 && q == 0;
    ps.user_init = d_user_init != nullptr;
    ps.cg = !ps.ar_only && method == ARIMA_METHOD_CSS_CGD && k > 0;
    ps.valid = true;
    return ARIMA_OK;
}

// The record of the call's next slice: the next slot of the ring, free to overwrite. More slices than slots: the slot's
// pending slice is the oldest of THIS call, and its stats are folded into the call's running total first.
static int take_slice_slot(arima_handle *h, FitRecord **rec) {
    SliceSlot &ss = h->slot[h->slot_seq++ % kSliceSlots];
    if (!ss.used) {
        RCCHK(h, ss.rec.create(), "slice events");
        ss.used = true;
    } else if (hipEventQuery(ss.rec.ev[4]) != hipSuccess) {
        HIPCHK(h, hipEventSynchronize(ss.rec.ev[4]));       // its previous slice's counter copy must have landed
    }
    if (h->slice_n == (unsigned)kSliceSlots) {
        acc_stats(h->slice_acc, ss.rec.stats());
        h->slice_first = (h->slice_first + 1) % kSliceSlots;
        h->slice_n--;
    }
    *rec = &ss.rec;
    return ARIMA_OK;
}

int arima_fit_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T, int64_t ld,
                           int32_t p, int32_t d, int32_t q, int32_t include_intercept, int32_t method,
                           const double *d_user_init, double *d_coef_out, double *d_css_ll_out,
                           int32_t *d_status_out, int32_t *d_n_eval_out, int32_t *d_n_grad_out,
                           uint8_t *d_flags_out, void *stream) {
    if (!h) return ARIMA_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    // (1) the argument checks: a refused call touches no device
    const FitOut out{d_coef_out, d_css_ll_out, d_status_out, d_n_eval_out, d_n_grad_out, d_flags_out};
    RCCHK(h, check_orders(h, p, d, q, include_intercept), "orders");
    if (n_series < 0 || T < 0 || ld < T) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    if (!out.coef || !out.ll || !out.status) return set_err(h, ARIMA_E_INVALID_ARG, "null output");
    const int P = h->pipeline, k = include_intercept + p + q;
    HIPCHK(h, hipSetDevice(h->device));
    // (2) the slice size: option fit_slice_bytes, or (0, the default) as large as the free HBM allows for P contexts.
    // Every slice ends with its own slowest series (the launch's critical path), so fewer, larger slices are faster
    // (C4 at 1M x 4096 in 262k-series slices: 2.9 s per fit alone, one slice: 1.2 s).
    int64_t slice_bytes = h->fit_slice_bytes;
    if (slice_bytes <= 0) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(h, hipMemGetInfo(&free_b, &total_b));
        size_t held = 0;                           // the contexts' differenced workspaces are reused
        for (int j = 0; j < P; ++j) held += h->fctx[j].diff.bytes;
        slice_bytes = std::max<int64_t>(1ll << 30, (int64_t)((free_b + held) / 10 * 6 / (size_t)std::max(P, 1)));
    }
    const int64_t slice = sts::plan::fit_slice_rows(slice_bytes, row_stride(h, T - d));
    // (3) the slices, each on the next fit context in the rotation (its own rows of the outputs), exactly as
    // consecutive calls. A call of one slice records into its context; a sliced one into the slots of the ring.
    const int64_t nslices = std::max<int64_t>(1, (n_series + slice - 1) / slice);
    const bool sliced = nslices > 1;
    h->stats = arima_fit_stats{};
    h->stats_from = sliced ? StatsFrom::kSlices : StatsFrom::kContext;
    if (sliced) {
        h->slice_first = h->slot_seq % kSliceSlots;
        h->slice_n = 0;
        h->slice_acc = arima_fit_stats{};
    }
    for (int64_t j = 0; j < nslices; ++j) {
        FitRecord *rec = nullptr;
        if (sliced) PASSCHK(take_slice_slot(h, &rec));
        const int ci = (int)(h->fit_seq++ % (unsigned)P);
        FitCtx &c = h->fctx[ci];
        if (!sliced) {
            rec = &c.rec;
            h->stats_ctx = ci;
        }
        const int64_t f = j * slice, ns = std::min(slice, n_series - f);
        const double *rows = d_series + f * ld, *uinit = d_user_init ? d_user_init + f * k : nullptr;
        const FitOut o = out.at(f, k);
        hipStream_t s = stream ? (hipStream_t)stream : c.stream;
        begin_fit(h, c, s);
        // hazards against in-flight fits of every context, whatever P is now: fits issued under a larger
        // fit_pipeline may still run on other contexts
        hipEvent_t ev_call = order_after_overlapping_fits(h, ci, call_spans(rows, ns, T, ld, k, uinit, o), s);
        int rc = fit_device_locked(h, c, *rec, P, rows, ns, T, ld, p, d, q, include_intercept, method, uinit, o, s,
                                   P > 1);
        // a slot's copy has landed once this event has passed (a context's record is waited for through ev_done)
        if (sliced && rc == ARIMA_OK && hipEventRecord(rec->ev[4], s) != hipSuccess)
            rc = set_err(h, ARIMA_E_DEVICE, "slice event");
        HIPCHK(h, end_fit(c, s));
        if (ev_call) HIPCHK(h, hipEventRecord(ev_call, s));
        if (sliced) h->slice_n++;
        if (rc != ARIMA_OK) return rc;
    }
    return ARIMA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Host path (end to end from host memory). The batch is cut into chunks of h->host_chunk
// series that rotate over h->host_pipeline contexts: chunk j's upload (from the caller's pageable buffer, staged by
// the HIP runtime) runs while the fits of chunks j-1, j-2 are still on the device, so PCIe and compute overlap and
// the tail of one chunk's fit kernel overlaps the next chunk's work. Results come back through pinned staging and
// are copied to the caller's arrays when the context is reused (or at the end).
// ---------------------------------------------------------------------------------------------------------
using sts::plan::pin_layout;   // one chunk's results in pinned staging (host_plan.hpp)

// Host rows -> device on stream s through the handle's ring of pinned blocks: block i is filled by the copy threads
// while block i-1's DMA runs; a block is refilled only after its previous DMA has finished (its event). The caller's
// buffer is fully read when this returns (as a pageable hipMemcpyAsync's is).
static int upload_staged(arima_handle *h, void *dst, const void *src, size_t bytes, hipStream_t s) {
    if (bytes == 0) return ARIMA_OK;
    if (h->host_copy_threads <= 0) {
        HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
        return ARIMA_OK;
    }
    for (size_t off = 0; off < bytes;) {
        const int j = (int)(h->stage_next++ % arima_handle::kStageSlots);
        if (!h->stage[j]) {
            if (hipHostMalloc(&h->stage[j], arima_handle::kStageBytes, 0) != hipSuccess)
                return set_err(h, ARIMA_E_OOM, "pinned staging");
            HIPCHK(h, hipEventCreateWithFlags(&h->stage_ev[j], hipEventDisableTiming));
        } else if (h->stage_used[j]) {
            HIPCHK(h, hipEventSynchronize(h->stage_ev[j]));
        }
        const size_t len = std::min(arima_handle::kStageBytes, bytes - off);
        sts::plan::par_memcpy(h->stage[j], (const char *)src + off, len, h->host_copy_threads);
        HIPCHK(h, hipMemcpyAsync((char *)dst + off, h->stage[j], len, hipMemcpyHostToDevice, s));
        HIPCHK(h, hipEventRecord(h->stage_ev[j], s));
        h->stage_used[j] = true;
        off += len;
    }
    return ARIMA_OK;
}

// Wait for context c's chunk, copy its results to the caller's arrays and add its counters to h->host_acc.
static int drain_chunk(arima_handle *h, FitCtx &c, int k, const FitOut &o) {
    if (c.chunk_n <= 0) return ARIMA_OK;
    HIPCHK(h, hipEventSynchronize(c.ev_done));
    const int64_t f = c.chunk_first, n = c.chunk_n;
    c.chunk_n = 0;
    // this chunk's own stats (zeros if its fit left none), never whatever h->stats holds from another chunk
    const bool kernel_counters = c.rec.ps.valid && c.rec.ps.cg;
    arima_fit_stats st = c.rec.stats();
    c.rec.ps.valid = false;
    size_t off[6];
    pin_layout(n, k, off);
    const char *b = static_cast<const char *>(c.pin);
    if (!kernel_counters) {
        // css-bobyqa, the AR-only shortcut and uniform status fills keep no device counters: the evaluation counts are
        // the sums of the per-series results, which are on the host already
        const int32_t *ne = reinterpret_cast<const int32_t *>(b + off[3]);
        const int32_t *ng = reinterpret_cast<const int32_t *>(b + off[4]);
        st.n_eval = st.n_grad = 0;
        for (int64_t i = 0; i < n; ++i) {
            st.n_eval += ne[i];
            st.n_grad += ng[i];
        }
        st.n_series = n;
    }
    acc_stats(h->host_acc, st);
    RCCHK(h, check_fault(h, c), "fault");
    if (k > 0) memcpy(o.coef + f * k, b + off[0], (size_t)n * k * 8);
    memcpy(o.ll + f, b + off[1], (size_t)n * 8);
    memcpy(o.status + f, b + off[2], (size_t)n * 4);
    if (o.n_eval) memcpy(o.n_eval + f, b + off[3], (size_t)n * 4);
    if (o.n_grad) memcpy(o.n_grad + f, b + off[4], (size_t)n * 4);
    if (o.flags) memcpy(o.flags + f, b + off[5], (size_t)n);
    return ARIMA_OK;
}

int arima_fit_batch(arima_handle *h, const double *series, int64_t N, int32_t T, int32_t p, int32_t d, int32_t q,
                    int32_t I, int32_t method, const double *user_init, double *coef_out, double *css_ll_out,
                    int32_t *status_out, int32_t *n_eval_out, int32_t *n_grad_out, uint8_t *flags_out) {
    if (!h) return ARIMA_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    RCCHK(h, check_orders(h, p, d, q, I), "orders");
    if (N < 0 || T < 0 || (N > 0 && (!series || !coef_out || !css_ll_out || !status_out)))
        return set_err(h, ARIMA_E_INVALID_ARG, "bad arguments");
    h->stats = arima_fit_stats{};
    h->stats_from = StatsFrom::kNone;
    if (N == 0) return ARIMA_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const int k = I + p + q;
    const int P = h->host_pipeline;
    // Chunk boundaries (host_plan.hpp): full chunks, then the last two chunks' worth halved again and again (down to
    // 16 384 series, never above host_chunk). The call ends with the fit of its last chunk, whose duration is that
    // chunk's slowest series: a small last chunk exposes less of it after the final upload (C2 1M x 1024 on 8 queues:
    // profiles/r06/g_e2e, h_e2e). Every buffer below is sized from the plan's largest chunk, whatever the schedule.
    const std::vector<int64_t> starts = sts::plan::host_chunk_starts(N, h->host_chunk, h->host_tail);
    const int64_t chunk = sts::plan::max_chunk(starts);
    const int64_t nchunks = (int64_t)starts.size() - 1;
    const int used = (int)std::min<int64_t>(P, nchunks);
    const FitOut o{coef_out, css_ll_out, status_out, n_eval_out, n_grad_out, flags_out};
    h->host_acc = arima_fit_stats{};
    // every context the call uses: settle what an earlier call left in it, then size its buffers for the largest chunk
    for (int j = 0; j < used; ++j) {
        FitCtx &c = h->fctx[j];
        if (c.has_done) HIPCHK(h, hipEventSynchronize(c.ev_done));
        c.chunk_n = 0;
        RCCHK(h, c.d_series.ensure((size_t)chunk * std::max(T, 1) * sizeof(double)), "staging");
        RCCHK(h, c.d_coef.ensure((size_t)chunk * std::max(k, 1) * sizeof(double)), "staging");
        RCCHK(h, c.d_ll.ensure((size_t)chunk * sizeof(double)), "staging");
        RCCHK(h, c.d_status.ensure((size_t)chunk * sizeof(int32_t)), "staging");
        RCCHK(h, c.d_neval.ensure((size_t)chunk * sizeof(int32_t)), "staging");
        RCCHK(h, c.d_ngrad.ensure((size_t)chunk * sizeof(int32_t)), "staging");
        RCCHK(h, c.d_flags.ensure((size_t)chunk), "staging");
        if (user_init) RCCHK(h, c.d_uinit.ensure((size_t)chunk * std::max(k, 1) * sizeof(double)), "staging");
        size_t off[6];
        const size_t need = pin_layout(chunk, k, off);
        if (c.pin_bytes < need) {
            if (c.pin) hipHostFree(c.pin);
            c.pin = nullptr;
            c.pin_bytes = 0;
            if (hipHostMalloc(&c.pin, need, 0) != hipSuccess) return set_err(h, ARIMA_E_OOM, "pinned staging");
            c.pin_bytes = need;
        }
    }
    int rc = ARIMA_OK;
    for (int64_t j = 0; j < nchunks && rc == ARIMA_OK; ++j) {
        const int ci = (int)(j % P);
        FitCtx &c = h->fctx[ci];
        rc = drain_chunk(h, c, k, o);                       // chunk j - P
        if (rc != ARIMA_OK) break;
        const int64_t first = starts[j], n = starts[j + 1] - starts[j];
        hipStream_t s = c.stream;
        begin_fit(h, c, s);
        if (T > 0) RCCHK(h, upload_staged(h, c.d_series.ptr, series + first * T, (size_t)n * T * sizeof(double), s),
                         "upload");
        const double *d_ui = nullptr;
        if (user_init) {
            if (k > 0)
                HIPCHK(h, hipMemcpyAsync(c.d_uinit.ptr, user_init + first * k, (size_t)n * k * sizeof(double),
                                         hipMemcpyHostToDevice, s));
            d_ui = c.d_uinit.as<double>();
        }
        rc = fit_device_locked(h, c, c.rec, used, c.d_series.as<double>(), n, T, T, p, d, q, I, method, d_ui,
                               c.dev_out(), s, nchunks > 1);
        if (rc == ARIMA_OK) {
            size_t off[6];
            pin_layout(n, k, off);
            char *b = static_cast<char *>(c.pin);
            if (k > 0) HIPCHK(h, hipMemcpyAsync(b + off[0], c.d_coef.ptr, (size_t)n * k * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(h, hipMemcpyAsync(b + off[1], c.d_ll.ptr, (size_t)n * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(h, hipMemcpyAsync(b + off[2], c.d_status.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(h, hipMemcpyAsync(b + off[3], c.d_neval.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(h, hipMemcpyAsync(b + off[4], c.d_ngrad.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(h, hipMemcpyAsync(b + off[5], c.d_flags.ptr, (size_t)n, hipMemcpyDeviceToHost, s));
            c.chunk_first = first;
            c.chunk_n = n;
        }
        HIPCHK(h, end_fit(c, s));
    }
    for (int j = 0; j < used; ++j) {                        // the last chunks (every context, even after an error)
        const int r = drain_chunk(h, h->fctx[j], k, o);
        if (rc == ARIMA_OK) rc = r;
    }
    h->stats = h->host_acc;
    const int rf = take_fault(h);          // already reported per chunk when set: clear the sticky record
    return rc != ARIMA_OK ? rc : rf;
}

// ---------------------------------------------------------------------------------------------------------
// building blocks (host buffers)
// ---------------------------------------------------------------------------------------------------------
int arima_difference_batch(arima_handle *h, const double *series, int64_t N, int32_t T, int32_t d, double *out) {
    if (!h || N < 0 || T < 0 || d < 0) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, kHostBuffers);
    if (N == 0 || T == 0) return ARIMA_OK;
    PASSCHK(f.begin());
    const size_t bytes = (size_t)N * T * sizeof(double);
    PASSCHK(f.stage({buf_in(series, bytes), buf_out(out, bytes)}));
    RCCHK(h, sts::launch_difference(f.dev<double>(0), T, f.dev<double>(1), T, N, T, d, 0, f.s()), "difference");
    return f.finish();
}

int arima_inverse_difference_batch(arima_handle *h, const double *series, int64_t N, int32_t T, int32_t d,
                                   double *out) {
    if (!h || N < 0 || T < 0 || d < 0) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, kHostBuffers);
    if (N == 0 || T == 0) return ARIMA_OK;
    PASSCHK(f.begin());
    const size_t bytes = (size_t)N * T * sizeof(double);
    PASSCHK(f.stage({buf_in(series, bytes), buf_out(out, bytes)}));
    RCCHK(h, sts::launch_inverse_difference(f.dev<double>(0), T, f.dev<double>(1), T, N, T, d, f.s()),
          "inverse_difference");
    return f.finish();
}

// upload N rows of length n into the padded (ld multiple of 16) workspace h->diff
static int upload_padded(arima_handle *h, const double *src, int64_t N, int32_t n, int64_t *ld_out, hipStream_t s) {
    const int64_t ld = row_stride(h, n);
    RCCHK(h, h->diff.ensure((size_t)N * ld * sizeof(double)), "workspace");
    if (n > 0)
        HIPCHK(h, hipMemcpy2DAsync(h->diff.ptr, ld * sizeof(double), src, (size_t)n * sizeof(double),
                                   (size_t)n * sizeof(double), N, hipMemcpyHostToDevice, s));
    *ld_out = ld;
    return ARIMA_OK;
}

int arima_css_loglik_batch(arima_handle *h, const double *series, int64_t N, int32_t T, int32_t p, int32_t d,
                           int32_t q, int32_t I, const double *coef, double *ll_out) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, kHostBuffers);
    RCCHK(h, check_orders(h, p, d, q, I), "orders");
    if (N < 0 || T < 0) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    if (N == 0) return ARIMA_OK;
    PASSCHK(f.begin());
    const int k = I + p + q;
    const int n = std::max(T - d, 0);
    const int64_t ldn = row_stride(h, n);
    RCCHK(h, h->diff.ensure((size_t)N * ldn * sizeof(double)), "workspace");
    PASSCHK(f.stage({buf_in(series, (size_t)N * T * sizeof(double)), buf_in(coef, (size_t)N * k * sizeof(double)),
                     buf_out(ll_out, (size_t)N * sizeof(double))}));
    RCCHK(h, sts::launch_difference(f.dev<double>(0), T, h->diff.as<double>(), ldn, N, T, d, 1, f.s()), "difference");
    RCCHK(h, sts::launch_css_loglik(h->diff.as<double>(), ldn, n, N, p, q, I, f.dev<double>(1), f.dev<double>(2),
                                    f.s()), "css_loglik");
    return f.finish();
}

int arima_css_gradient_batch(arima_handle *h, const double *diffed, int64_t N, int32_t n, int32_t p, int32_t q,
                             int32_t I, const double *coef, double *grad_out) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, kHostBuffers);
    RCCHK(h, check_orders(h, p, 0, q, I), "orders");
    if (N < 0 || n < 0) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    const int k = I + p + q;
    if (N == 0 || k == 0) return ARIMA_OK;
    PASSCHK(f.begin());
    int64_t ld = 0;
    RCCHK(h, upload_padded(h, diffed, N, n, &ld, f.s()), "upload");
    const size_t coef_bytes = (size_t)N * k * sizeof(double);
    PASSCHK(f.stage({buf_in(coef, coef_bytes), buf_out(grad_out, coef_bytes)}));
    RCCHK(h, sts::launch_css_grad(h->diff.as<double>(), ld, n, N, p, q, I, h->smear, f.dev<double>(0), f.dev<double>(1),
                                  f.s()), "css_grad");
    return f.finish();
}

int arima_hannan_rissanen_batch(arima_handle *h, const double *diffed, int64_t N, int32_t n, int32_t p, int32_t q,
                                int32_t I, double *init_out, int32_t *status_out) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, kHostBuffers);
    RCCHK(h, check_orders(h, p, 0, q, I), "orders");
    if (N < 0 || n < 0) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    if (N == 0) return ARIMA_OK;
    PASSCHK(f.begin());
    const int k = I + p + q;
    int64_t ld = 0;
    RCCHK(h, upload_padded(h, diffed, N, n, &ld, f.s()), "upload");
    PASSCHK(f.stage({buf_out(init_out, (size_t)N * k * sizeof(double)),
                     buf_out(status_out, (size_t)N * sizeof(int32_t))}));
    RCCHK(h, sts::launch_hr_init(h->diff.as<double>(), ld, n, N, p, q, I, f.dev<double>(0), f.dev<int32_t>(1), f.s(),
                                 std::max(h->hr_grid, 0)), "hr_init");
    return f.finish();
}

int arima_model_flags_batch(arima_handle *h, const double *coef, int64_t N, int32_t p, int32_t q, int32_t I,
                            uint8_t *flags_out) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, kHostBuffers);
    RCCHK(h, check_orders(h, p, 0, q, I), "orders");
    if (N <= 0) return ARIMA_OK;
    PASSCHK(f.begin());
    PASSCHK(f.stage({buf_in(coef, (size_t)N * (I + p + q) * sizeof(double)), buf_out(flags_out, (size_t)N)}));
    RCCHK(h, sts::launch_model_flags(f.dev<double>(0), N, p, q, I, f.dev<uint8_t>(1), f.s()), "flags");
    return f.finish();
}

// ARIMAModel.forecast over a device batch: k_forecast (p, q <= 5, d <= 8, the streaming kernel) or the runtime-order
// k_gen_forecast for every other order
static int forecast_any(arima_handle *h, const double *ts, int64_t ld, const double *coef, int k, double *out,
                        int64_t ld_out, int64_t N, int T, int p, int d, int q, int I, int n_future, hipStream_t s) {
    if (!sts::gen_order(p, q) && d <= 8)
        return sts::launch_forecast(ts, ld, coef, k, out, ld_out, N, T, p, d, q, I, n_future, s);
    const int64_t w = sts::gen_forecast_ws_doubles(T, p, d, q, n_future);
    return forecast_slices(h, N, w, "forecast", [&](int64_t f, int64_t m, double *ws) {
        return sts::launch_gen_forecast(ts + f * ld, ld, coef + f * k, k, out + f * ld_out, ld_out, m, T, p, d, q, I,
                                        n_future, ws, w, s);
    });
}

// From here on the two flavours of an operation share one body (the ARIMA effects pair excepted): the host flavour is
// the device flavour at dense strides, on the handle's stream, over the staged copies of its arrays (CallFrame).
static int forecast_body(arima_handle *h, CallFlavour flavour, const double *series, int64_t N, int32_t T, int64_t ld,
                         int32_t p, int32_t d, int32_t q, int32_t I, const double *coef, int32_t n_future, double *out,
                         int64_t ld_out, void *stream) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, flavour);
    RCCHK(h, check_orders(h, p, d, q, I), "orders");
    if (N < 0 || T < d || n_future < 0 || ld < T || ld_out < (int64_t)T + n_future)
        return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    if (N == 0) return ARIMA_OK;
    const int k = I + p + q;
    PASSCHK(f.bind({buf_in(series, strided_bytes(N, ld, T)), buf_in(coef, N * k * (int64_t)sizeof(double)),
                    buf_out(out, strided_bytes(N, ld_out, (int64_t)T + n_future))}));
    PASSCHK(f.begin(stream));
    RCCHK(h, forecast_any(h, f.dev<double>(0), ld, f.dev<double>(1), k, f.dev<double>(2), ld_out, N, T, p, d, q, I,
                          n_future, f.s()), "forecast");
    return f.finish();
}

int arima_forecast_batch(arima_handle *h, const double *series, int64_t N, int32_t T, int32_t p, int32_t d,
                         int32_t q, int32_t I, const double *coef, int32_t n_future, double *out) {
    return forecast_body(h, kHostBuffers, series, N, T, T, p, d, q, I, coef, n_future, out, (int64_t)T + n_future, nullptr);
}

int arima_forecast_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                int32_t p, int32_t d, int32_t q, int32_t I, const double *d_coef, int32_t n_future,
                                double *d_out, int64_t ld_out, void *stream) {
    return forecast_body(h, kDeviceBuffers, d_series, N, T, ld, p, d, q, I, d_coef, n_future, d_out, ld_out, stream);
}


// ARIMAModel.removeTimeDependentEffects / addTimeDependentEffects over a device batch: k_effects (p, q <= 5, d <= 8,
// the tiled streaming kernel) or the runtime-order k_gen_effects for every other order
static int effects_any(const double *in, int64_t ld, const double *coef, int k, double *out, int64_t ld_out,
                       int64_t N, int T, int p, int d, int q, int I, int add, hipStream_t s) {
    if (!sts::gen_order(p, q) && d <= 8)
        return sts::launch_effects(in, ld, coef, k, out, ld_out, N, T, p, d, q, I, add, s);
    return sts::launch_gen_effects(in, ld, coef, k, out, ld_out, N, T, p, d, q, I, add, s);
}

// The ARIMA effects pair may run in place (`aliased`: the output IS the input, same start and stride); any other
// meeting of the output with the rows or the coefficients is refused.
static int effects_overlap(arima_handle *h, ByteSpan in, ByteSpan coef, ByteSpan out, bool aliased) {
    const ByteSpan ins[2] = {aliased ? ByteSpan() : in, coef};
    if (sts::plan::find_overlap(ins, 2, &out, 1)) return set_err(h, ARIMA_E_INVALID_ARG, "out overlaps an input");
    return ARIMA_OK;
}

// This pair keeps a body per flavour: the host flavour stages the rows once, runs in place on them and downloads them
// into `out`, so its output has no region and no row of its own, while the device flavour has two strided buffers.
static int effects_host(arima_handle *h, const double *in, int64_t N, int32_t T, int32_t p, int32_t d, int32_t q,
                        int32_t I, const double *coef, double *out, int add) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, kHostBuffers);
    RCCHK(h, check_orders(h, p, d, q, I), "orders");
    if (N < 0 || T < d) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    if (N == 0 || T == 0) return ARIMA_OK;
    const int k = I + p + q;
    if (!in || (!coef && k > 0) || !out) return set_err(h, ARIMA_E_INVALID_ARG, "null buffer");
    const size_t row_bytes = (size_t)N * T * sizeof(double), coef_bytes = (size_t)N * k * sizeof(double);
    PASSCHK(effects_overlap(h, ByteSpan(in, row_bytes), ByteSpan(coef, coef_bytes), ByteSpan(out, row_bytes),
                            out == in));
    PASSCHK(f.begin());
    PASSCHK(f.stage({buf_in(in, row_bytes), buf_in(coef, coef_bytes)}));
    // in place on the staged rows: every wave reads a tile before it writes it
    RCCHK(h, effects_any(f.dev<double>(0), T, f.dev<double>(1), k, f.dev<double>(0), T, N, T, p, d, q, I, add, f.s()),
          "effects");
    return f.finish(f.download(0, out));
}

static int effects_device(arima_handle *h, const double *d_in, int64_t N, int32_t T, int64_t ld, int32_t p, int32_t d,
                          int32_t q, int32_t I, const double *d_coef, double *d_out, int64_t ld_out, void *stream,
                          int add) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, kDeviceBuffers);
    RCCHK(h, check_orders(h, p, d, q, I), "orders");
    if (N < 0 || T < d || ld < T || ld_out < T) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    if (N == 0 || T == 0) return ARIMA_OK;
    const int k = I + p + q;
    if (!d_in || (!d_coef && k > 0) || !d_out) return set_err(h, ARIMA_E_INVALID_ARG, "null buffer");
    PASSCHK(effects_overlap(h, ByteSpan(d_in, ((N - 1) * ld + T) * (int64_t)sizeof(double)),
                            ByteSpan(d_coef, N * k * (int64_t)sizeof(double)),
                            ByteSpan(d_out, ((N - 1) * ld_out + T) * (int64_t)sizeof(double)),
                            d_out == d_in && ld_out == ld));
    PASSCHK(f.begin(stream));
    RCCHK(h, effects_any(d_in, ld, d_coef, k, d_out, ld_out, N, T, p, d, q, I, add, f.s()), "effects");
    return f.finish();
}

int arima_remove_effects_batch(arima_handle *h, const double *series, int64_t N, int32_t T, int32_t p, int32_t d,
                               int32_t q, int32_t I, const double *coef, double *out) {
    return effects_host(h, series, N, T, p, d, q, I, coef, out, 0);
}

int arima_add_effects_batch(arima_handle *h, const double *noise, int64_t N, int32_t T, int32_t p, int32_t d,
                            int32_t q, int32_t I, const double *coef, double *out) {
    return effects_host(h, noise, N, T, p, d, q, I, coef, out, 1);
}

int arima_remove_effects_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                      int32_t p, int32_t d, int32_t q, int32_t I, const double *d_coef, double *d_out,
                                      int64_t ld_out, void *stream) {
    return effects_device(h, d_series, N, T, ld, p, d, q, I, d_coef, d_out, ld_out, stream, 0);
}

int arima_add_effects_batch_device(arima_handle *h, const double *d_noise, int64_t N, int32_t T, int64_t ld,
                                   int32_t p, int32_t d, int32_t q, int32_t I, const double *d_coef, double *d_out,
                                   int64_t ld_out, void *stream) {
    return effects_device(h, d_noise, N, T, ld, p, d, q, I, d_coef, d_out, ld_out, stream, 1);
}

// ---------------------------------------------------------------------------------------------------------
// residual diagnostics: autocorr, dwtest, lbtest per row (arima_diag.hip), over given rows or over the residuals of
// fitted models without handing the N x T residuals to the caller
// ---------------------------------------------------------------------------------------------------------
namespace {
struct DiagOut {
    double *acf, *dw, *lbs, *lbp;
    bool lags() const { return acf || lbs || lbp; }
    bool any() const { return lags() || dw; }
};

// shape and lag rules shared by the four entry points; *done: nothing to compute (ARIMA_OK)
int diag_check(arima_handle *h, int64_t N, int32_t T, int32_t max_lag, const DiagOut &o, bool *done) {
    *done = false;
    if (N < 0 || T < 0) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    if (N == 0 || T == 0 || !o.any()) {
        *done = true;
        return ARIMA_OK;
    }
    // the reference's slicing (UnivariateTimeSeries.scala:75-76) and ChiSquaredDistribution(0) throw
    if (o.lags() && (max_lag < 1 || max_lag > T - 1)) return set_err(h, ARIMA_E_INVALID_ARG, "max_lag outside [1, T - 1]");
    return ARIMA_OK;
}

// The byte budget of one slice of a sliced call's workspace: the option's value if positive, else 60 % of the free HBM
// plus what the workspace already holds (`held`), at least 1 GiB
int auto_slice_bytes(arima_handle *h, int64_t option, size_t held, int64_t *slice_bytes) {
    *slice_bytes = option;
    if (option > 0) return ARIMA_OK;
    size_t free_b = 0, total_b = 0;
    HIPCHK(h, hipMemGetInfo(&free_b, &total_b));
    *slice_bytes = std::max<int64_t>(1ll << 30, (int64_t)((free_b + held) / 10 * 6));
    return ARIMA_OK;
}

// removeTimeDependentEffects into a bounded workspace slice, then the diagnostics of that slice, slice by slice
int residual_diag_dev(arima_handle *h, const double *d_series, int64_t N, int T, int64_t ld, int p, int d, int q, int I,
                      const double *d_coef, int max_lag, const DiagOut &o, hipStream_t s) {
    const int k = I + p + q;
    const int64_t ldw = round_up(T, 16);                      // 128-B aligned residual rows
    int64_t slice_bytes;
    PASSCHK(auto_slice_bytes(h, h->diag_slice_bytes, h->dg_resid.bytes, &slice_bytes));
    const int64_t slice = sts::plan::diag_slice_rows(slice_bytes, ldw);
    RCCHK(h, h->dg_resid.ensure((size_t)std::min(slice, N) * ldw * sizeof(double)), "residual workspace");
    double *resid = h->dg_resid.as<double>();
    for (int64_t f = 0; f < N; f += slice) {
        const int64_t n = std::min(slice, N - f);
        RCCHK(h, effects_any(d_series + f * ld, ld, d_coef + f * k, k, resid, ldw, n, T, p, d, q, I, 0, s), "effects");
        RCCHK(h, sts::launch_diag(resid, ldw, n, T, max_lag, o.acf ? o.acf + f * max_lag : nullptr,
                                  o.dw ? o.dw + f : nullptr, o.lbs ? o.lbs + f : nullptr,
                                  o.lbp ? o.lbp + f : nullptr, s), "diagnostics");
    }
    return ARIMA_OK;
}
}  // namespace

static int diag_body(arima_handle *h, CallFlavour flavour, const double *rows, int64_t N, int32_t T, int64_t ld,
                     int32_t max_lag, const DiagOut &o, void *stream) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, flavour);
    if (ld < T) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    bool done;
    RCCHK(h, diag_check(h, N, T, max_lag, o, &done), "diagnostics");
    if (done) return ARIMA_OK;
    const int64_t nd = N * (int64_t)sizeof(double);
    PASSCHK(f.bind({buf_in(rows, strided_bytes(N, ld, T)), buf_opt_out(o.acf, nd * max_lag), buf_opt_out(o.dw, nd),
                    buf_opt_out(o.lbs, nd), buf_opt_out(o.lbp, nd)}));
    RCCHK(h, f.overlap(), "overlap");
    PASSCHK(f.begin(stream));
    RCCHK(h, sts::launch_diag(f.dev<double>(0), ld, N, T, max_lag, f.dev<double>(1), f.dev<double>(2), f.dev<double>(3),
                              f.dev<double>(4), f.s()), "diagnostics");
    return f.finish();
}

int arima_diagnostics_batch(arima_handle *h, const double *rows, int64_t N, int32_t T, int32_t max_lag,
                            double *acf_out, double *dw_out, double *lb_stat_out, double *lb_pvalue_out) {
    return diag_body(h, kHostBuffers, rows, N, T, T, max_lag, {acf_out, dw_out, lb_stat_out, lb_pvalue_out}, nullptr);
}

int arima_diagnostics_batch_device(arima_handle *h, const double *d_rows, int64_t N, int32_t T, int64_t ld,
                                   int32_t max_lag, double *d_acf_out, double *d_dw_out, double *d_lb_stat_out,
                                   double *d_lb_pvalue_out, void *stream) {
    return diag_body(h, kDeviceBuffers, d_rows, N, T, ld, max_lag,
                     {d_acf_out, d_dw_out, d_lb_stat_out, d_lb_pvalue_out}, stream);
}

static int residual_diag_body(arima_handle *h, CallFlavour flavour, const double *series, int64_t N, int32_t T,
                              int64_t ld, int32_t p, int32_t d, int32_t q, int32_t I, const double *coef,
                              int32_t max_lag, const DiagOut &o, void *stream) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, flavour);
    RCCHK(h, check_orders(h, p, d, q, I), "orders");
    if (T < d || ld < T) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    bool done;
    RCCHK(h, diag_check(h, N, T, max_lag, o, &done), "diagnostics");
    if (done) return ARIMA_OK;
    const int k = I + p + q;
    const int64_t nd = N * (int64_t)sizeof(double);
    PASSCHK(f.bind({buf_in(series, strided_bytes(N, ld, T)), buf_in(coef, nd * k, k > 0),
                    buf_opt_out(o.acf, nd * max_lag), buf_opt_out(o.dw, nd), buf_opt_out(o.lbs, nd),
                    buf_opt_out(o.lbp, nd)}));
    RCCHK(h, f.overlap(), "overlap");
    PASSCHK(f.begin(stream));
    const DiagOut dev{f.dev<double>(2), f.dev<double>(3), f.dev<double>(4), f.dev<double>(5)};
    RCCHK(h, residual_diag_dev(h, f.dev<double>(0), N, T, ld, p, d, q, I, f.dev<double>(1), max_lag, dev, f.s()),
          "residual diagnostics");
    return f.finish();
}

int arima_residual_diagnostics_batch(arima_handle *h, const double *series, int64_t N, int32_t T, int32_t p,
                                     int32_t d, int32_t q, int32_t I, const double *coef, int32_t max_lag,
                                     double *acf_out, double *dw_out, double *lb_stat_out, double *lb_pvalue_out) {
    return residual_diag_body(h, kHostBuffers, series, N, T, T, p, d, q, I, coef, max_lag,
                              {acf_out, dw_out, lb_stat_out, lb_pvalue_out}, nullptr);
}

int arima_residual_diagnostics_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                            int32_t p, int32_t d, int32_t q, int32_t I, const double *d_coef,
                                            int32_t max_lag, double *d_acf_out, double *d_dw_out,
                                            double *d_lb_stat_out, double *d_lb_pvalue_out, void *stream) {
    return residual_diag_body(h, kDeviceBuffers, d_series, N, T, ld, p, d, q, I, d_coef, max_lag,
                              {d_acf_out, d_dw_out, d_lb_stat_out, d_lb_pvalue_out}, stream);
}

// ---------------------------------------------------------------------------------------------------------
// regressions over a design matrix (arima_regress.hip): AutoregressionX.fitModel, ARXModel.predict, bgtest, bptest
// ---------------------------------------------------------------------------------------------------------
namespace {
using sts::RgDesign;
using sts::RgSrc;

// What commons' validateSampleData and newXSampleData (and, before them, the reference's slicing) throw for a shape,
// the same for every series of the call, in orc_ols's order
int32_t regress_shape_status(const RgDesign &d) {
    const int R = d.rows();
    if (R < 0) return ARIMA_ST_SERIES_TOO_SHORT;
    if (R == 0) return ARIMA_ST_NO_DATA;
    if (d.num_pred() + 1 > R) return ARIMA_ST_NOT_ENOUGH_DATA;
    if (d.cols() == 0) return ARIMA_ST_NO_DATA;
    return ARIMA_ST_OK;
}

// argument rules shared by the eight entry points; *done: nothing to compute (ARIMA_OK)
int regress_check(arima_handle *h, const RgDesign &d, int64_t N, int64_t ld, int64_t xs, bool *done) {
    *done = false;
    if (N < 0 || d.T < 0 || ld < d.T || d.k < 0 || d.lag_a < 0 || d.lag_b < 0)
        return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    // ChiSquaredDistribution(0) throws
    if (d.kind == sts::kRgBg && d.lag_a < 1) return set_err(h, ARIMA_E_INVALID_ARG, "max_lag < 1");
    if (d.kind == sts::kRgBp && d.k < 1) return set_err(h, ARIMA_E_INVALID_ARG, "n_xcols < 1");
    if (xs != 0 && xs < (int64_t)d.k * d.T) return set_err(h, ARIMA_E_INVALID_ARG, "x_series_stride below n_xcols * T");
    if (d.num_pred() + (d.icpt ? 1 : 0) > sts::kRgMaxCols) return set_err(h, ARIMA_E_UNSUPPORTED, "at most 64 columns");
    *done = N == 0;
    return ARIMA_OK;
}

// The caller's regressor block as a table row: one matrix of x_doubles values, or N of them x_series_stride apart. A
// block without values may be null.
Buf x_block(const double *x, int64_t x_doubles, int64_t N, int64_t xs) {
    const int64_t bytes = strided_bytes(xs ? N : 1, xs, x_doubles);
    return buf_in(x, bytes, bytes > 0);
}

// What the design kernels read, for the entry points whose table starts with the rows and the regressor block; a
// block without values is null for them
RgSrc rg_src(const CallFrame &f, int64_t ld, int64_t xs) {
    return {f.dev<double>(0), ld, f.bytes(1) ? f.dev<double>(1) : nullptr, xs};
}

// The fit (coef_out: N x (1 + K)) or the test (stat_out, pvalue_out: N) of every series, slice by slice: assemble, QR
// and, for a test, assemble again and calculateRSquared
int regress_dev(arima_handle *h, const RgDesign &d, const RgSrc &src, int64_t N, double *coef_out, double *stat_out,
                double *pvalue_out, int32_t *status_out, hipStream_t s) {
    const bool test = d.kind != sts::kRgArx;
    const int K = (int)d.num_pred(), C = d.cols(), R = d.rows();
    const int32_t shape = regress_shape_status(d);
    if (shape != ARIMA_ST_OK) {
        RCCHK(h, sts::launch_regress_refuse(N, shape, status_out, test ? stat_out : coef_out, test ? 1 : 1 + K,
                                            test ? pvalue_out : nullptr, 1, s), "regression");
        return ARIMA_OK;
    }
    int64_t slice_bytes;
    PASSCHK(auto_slice_bytes(h, h->regress_slice_bytes, h->rg_ws.bytes, &slice_bytes));
    const int64_t slice = sts::plan::regress_slice_rows(slice_bytes, (int64_t)(C + 1) * R);
    RCCHK(h, h->rg_ws.ensure((size_t)sts::rg_ws_doubles(std::min(slice, N), R, C) * sizeof(double)),
          "regression workspace");
    if (test) RCCHK(h, h->rg_beta.ensure((size_t)std::min(slice, N) * C * sizeof(double)), "regression workspace");
    double *ws = h->rg_ws.as<double>(), *beta = h->rg_beta.as<double>();
    for (int64_t f = 0; f < N; f += slice) {
        const int64_t n = std::min(slice, N - f);
        RCCHK(h, sts::launch_regress_assemble(d, src.at(f), n, ws, s), "design");
        if (!test) {
            RCCHK(h, sts::launch_regress_qr(ws, n, R, C, coef_out + f * (1 + K), 1 + K, d.icpt ? 0 : 1, d.icpt ? 0 : 1,
                                            status_out + f, s), "qr");
            continue;
        }
        RCCHK(h, sts::launch_regress_qr(ws, n, R, C, beta, C, 0, 0, status_out + f, s), "qr");
        RCCHK(h, sts::launch_regress_assemble(d, src.at(f), n, ws, s), "design");   // the QR ran in place
        // nObs = T - maxLag (bgtest), T (bptest): the rows; df = maxLag, k
        RCCHK(h, sts::launch_regress_r2(ws, beta, status_out + f, n, R, C, R, d.kind == sts::kRgBg ? d.lag_a : d.k,
                                        stat_out + f, pvalue_out + f, s), "r squared");
    }
    return ARIMA_OK;
}

// AutoregressionX.fitModel (coef_out) or a test (stat_out, pvalue_out); the pointers of the other kind are null
int regress_body(arima_handle *h, CallFlavour flavour, const RgDesign &d, const double *rows, int64_t N, int64_t ld,
                 const double *xreg, int64_t xs, double *coef_out, double *stat_out, double *pvalue_out,
                 int32_t *status_out, void *stream) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, flavour);
    bool done;
    PASSCHK(regress_check(h, d, N, ld, xs, &done));
    if (done) return ARIMA_OK;
    const bool test = d.kind != sts::kRgArx;
    const int64_t nd = N * (int64_t)sizeof(double);
    PASSCHK(f.bind({buf_in(rows, strided_bytes(N, ld, d.T), d.T > 0), x_block(xreg, (int64_t)d.k * d.T, N, xs),
                    test ? buf_out(stat_out, nd) : buf_out(coef_out, nd * (1 + d.num_pred())),
                    test ? buf_out(pvalue_out, nd) : buf_opt_out(nullptr, 0),
                    buf_out(status_out, N * (int64_t)sizeof(int32_t))}));
    PASSCHK(f.overlap());
    PASSCHK(f.begin(stream));
    PASSCHK(regress_dev(h, d, rg_src(f, ld, xs), N, test ? nullptr : f.dev<double>(2), test ? f.dev<double>(2) : nullptr,
                        f.dev<double>(3), f.dev<int32_t>(4), f.s()));
    return f.finish();
}

RgDesign arx_design(int32_t T, int32_t k, int32_t y_max_lag, int32_t x_max_lag, int32_t orig, int32_t no_intercept) {
    return {sts::kRgArx, T, k, y_max_lag, x_max_lag, orig ? 1 : 0, no_intercept ? 0 : 1};
}

// ARXModel.predict's own rule on top of regress_check: the reference's slicing throws for T < maxLag
int predict_check(arima_handle *h, const RgDesign &d, int64_t N, int64_t ld, int64_t xs, int64_t ld_out, bool *done) {
    PASSCHK(regress_check(h, d, N, ld, xs, done));
    if (d.rows() < 0 || ld_out < d.rows()) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    *done = *done || d.rows() == 0;
    return ARIMA_OK;
}
}  // namespace

int arima_arx_num_coef(int32_t n_xcols, int32_t y_max_lag, int32_t x_max_lag, int32_t include_original_x) {
    if (n_xcols < 0 || y_max_lag < 0 || x_max_lag < 0) return ARIMA_E_INVALID_ARG;
    const int64_t K = arx_design(0, n_xcols, y_max_lag, x_max_lag, include_original_x, 1).num_pred();
    return K > INT32_MAX ? ARIMA_E_INVALID_ARG : (int)K;
}

int arima_arx_fit_batch(arima_handle *h, const double *series, int64_t N, int32_t T, const double *xreg,
                        int64_t x_series_stride, int32_t n_xcols, int32_t y_max_lag, int32_t x_max_lag,
                        int32_t include_original_x, int32_t no_intercept, double *coef_out, int32_t *status_out) {
    return regress_body(h, kHostBuffers, arx_design(T, n_xcols, y_max_lag, x_max_lag, include_original_x, no_intercept),
                        series, N, T, xreg, x_series_stride, coef_out, nullptr, nullptr, status_out, nullptr);
}

int arima_arx_fit_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                               const double *d_xreg, int64_t x_series_stride, int32_t n_xcols, int32_t y_max_lag,
                               int32_t x_max_lag, int32_t include_original_x, int32_t no_intercept, double *d_coef_out,
                               int32_t *d_status_out, void *stream) {
    return regress_body(h, kDeviceBuffers,
                        arx_design(T, n_xcols, y_max_lag, x_max_lag, include_original_x, no_intercept), d_series, N, ld,
                        d_xreg, x_series_stride, d_coef_out, nullptr, nullptr, d_status_out, stream);
}

static int predict_body(arima_handle *h, CallFlavour flavour, const RgDesign &d, const double *series, int64_t N,
                        int64_t ld, const double *xreg, int64_t xs, const double *coef, double *out, int64_t ld_out,
                        void *stream) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, flavour);
    bool done;
    PASSCHK(predict_check(h, d, N, ld, xs, ld_out, &done));
    if (done) return ARIMA_OK;
    PASSCHK(f.bind({buf_in(series, strided_bytes(N, ld, d.T), d.T > 0), x_block(xreg, (int64_t)d.k * d.T, N, xs),
                    buf_in(coef, N * (1 + d.num_pred()) * (int64_t)sizeof(double)),
                    buf_out(out, strided_bytes(N, ld_out, d.rows()))}));
    PASSCHK(f.overlap());
    PASSCHK(f.begin(stream));
    RCCHK(h, sts::launch_arx_predict(d, rg_src(f, ld, xs), f.dev<double>(2), f.dev<double>(3), ld_out, N, f.s()),
          "predict");
    return f.finish();
}

int arima_arx_predict_batch(arima_handle *h, const double *series, int64_t N, int32_t T, const double *xreg,
                            int64_t x_series_stride, int32_t n_xcols, int32_t y_max_lag, int32_t x_max_lag,
                            int32_t include_original_x, const double *coef, double *out) {
    const RgDesign d = arx_design(T, n_xcols, y_max_lag, x_max_lag, include_original_x, 1);
    return predict_body(h, kHostBuffers, d, series, N, T, xreg, x_series_stride, coef, out, d.rows(), nullptr);
}

int arima_arx_predict_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                   const double *d_xreg, int64_t x_series_stride, int32_t n_xcols, int32_t y_max_lag,
                                   int32_t x_max_lag, int32_t include_original_x, const double *d_coef, double *d_out,
                                   int64_t ld_out, void *stream) {
    return predict_body(h, kDeviceBuffers, arx_design(T, n_xcols, y_max_lag, x_max_lag, include_original_x, 1), d_series,
                        N, ld, d_xreg, x_series_stride, d_coef, d_out, ld_out, stream);
}

int arima_bgtest_batch(arima_handle *h, const double *residuals, int64_t N, int32_t T, const double *factors,
                       int64_t x_series_stride, int32_t n_xcols, int32_t max_lag, double *stat_out, double *pvalue_out,
                       int32_t *status_out) {
    return regress_body(h, kHostBuffers, {sts::kRgBg, T, n_xcols, max_lag, 0, 0, 1}, residuals, N, T, factors,
                        x_series_stride, nullptr, stat_out, pvalue_out, status_out, nullptr);
}

int arima_bgtest_batch_device(arima_handle *h, const double *d_residuals, int64_t N, int32_t T, int64_t ld,
                              const double *d_factors, int64_t x_series_stride, int32_t n_xcols, int32_t max_lag,
                              double *d_stat_out, double *d_pvalue_out, int32_t *d_status_out, void *stream) {
    return regress_body(h, kDeviceBuffers, {sts::kRgBg, T, n_xcols, max_lag, 0, 0, 1}, d_residuals, N, ld, d_factors,
                        x_series_stride, nullptr, d_stat_out, d_pvalue_out, d_status_out, stream);
}

int arima_bptest_batch(arima_handle *h, const double *residuals, int64_t N, int32_t T, const double *factors,
                       int64_t x_series_stride, int32_t n_xcols, double *stat_out, double *pvalue_out,
                       int32_t *status_out) {
    return regress_body(h, kHostBuffers, {sts::kRgBp, T, n_xcols, 0, 0, 0, 1}, residuals, N, T, factors,
                        x_series_stride, nullptr, stat_out, pvalue_out, status_out, nullptr);
}

int arima_bptest_batch_device(arima_handle *h, const double *d_residuals, int64_t N, int32_t T, int64_t ld,
                              const double *d_factors, int64_t x_series_stride, int32_t n_xcols, double *d_stat_out,
                              double *d_pvalue_out, int32_t *d_status_out, void *stream) {
    return regress_body(h, kDeviceBuffers, {sts::kRgBp, T, n_xcols, 0, 0, 0, 1}, d_residuals, N, ld, d_factors,
                        x_series_stride, nullptr, d_stat_out, d_pvalue_out, d_status_out, stream);
}

// RegressionARIMA.fitCochraneOrcutt (RegressionARIMA.scala:83-160): regress_check's rules on the pristine-copy design,
// then its own
namespace {
int co_check(arima_handle *h, const RgDesign &d, int64_t N, int64_t ld, int64_t xs, int32_t max_iter, bool *done) {
    *done = false;
    // new Array(maxIter) or rhos(0) throws; the zero-column dgemv is unread
    if (max_iter < 1) return set_err(h, ARIMA_E_INVALID_ARG, "max_iter < 1");
    if (d.k < 1) return set_err(h, ARIMA_E_INVALID_ARG, "n_xcols < 1");
    PASSCHK(regress_check(h, d, N, ld, xs, done));
    if (d.num_pred() + 1 > sts::kRgMaxCols) return set_err(h, ARIMA_E_UNSUPPORTED, "at most 64 columns");
    return ARIMA_OK;
}

// Slice by slice: the pristine copy of y and X, then the whole iteration in one launch. A slice's workspace is the
// copy ((k + 1) T doubles per series) and the working design ((k + 2) T) behind it.
int co_dev(arima_handle *h, const RgDesign &d, const RgSrc &src, int64_t N, int32_t max_iter, double *coef_out,
           double *rho_out, int32_t *n_iter_out, int32_t *status_out, hipStream_t s) {
    const int k = d.k, T = d.T;
    // step 1's OLSMultipleLinearRegression.validateSampleData, the same for every series of the call
    const int32_t shape = T == 0 ? ARIMA_ST_NO_DATA : k + 1 > T ? ARIMA_ST_NOT_ENOUGH_DATA : ARIMA_ST_OK;
    if (shape != ARIMA_ST_OK) {
        RCCHK(h, sts::launch_regress_refuse(N, shape, status_out, coef_out, 1 + k, rho_out, 1, s), "regression");
        if (n_iter_out) HIPCHK(h, hipMemsetAsync(n_iter_out, 0, (size_t)N * sizeof(int32_t), s));
        return ARIMA_OK;
    }
    int64_t slice_bytes;
    PASSCHK(auto_slice_bytes(h, h->regress_slice_bytes, h->rg_ws.bytes, &slice_bytes));
    const int64_t slice = sts::plan::regress_slice_rows(slice_bytes, (int64_t)(2 * k + 3) * T);
    const int64_t copy_doubles = sts::rg_ws_doubles(std::min(slice, N), T, k);
    RCCHK(h, h->rg_ws.ensure((size_t)(copy_doubles + sts::rg_ws_doubles(std::min(slice, N), T, k + 1)) *
                             sizeof(double)), "regression workspace");
    double *ps = h->rg_ws.as<double>(), *wk = ps + copy_doubles;
    for (int64_t f = 0; f < N; f += slice) {
        const int64_t n = std::min(slice, N - f);
        RCCHK(h, sts::launch_regress_assemble(d, src.at(f), n, ps, s), "design");
        RCCHK(h, sts::launch_cochrane_orcutt(ps, wk, n, T, k, max_iter, coef_out + f * (1 + k), rho_out + f,
                                             n_iter_out ? n_iter_out + f : nullptr, status_out + f, s),
              "cochrane-orcutt");
    }
    return ARIMA_OK;
}
}  // namespace

static int co_body(arima_handle *h, CallFlavour flavour, const double *series, int64_t N, int32_t T, int64_t ld,
                   const double *xreg, int64_t xs, int32_t n_xcols, int32_t max_iter, double *coef_out, double *rho_out,
                   int32_t *n_iter_out, int32_t *status_out, void *stream) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, flavour);
    const RgDesign d{sts::kRgCo, T, n_xcols, 0, 0, 0, 0};
    bool done;
    PASSCHK(co_check(h, d, N, ld, xs, max_iter, &done));
    if (done) return ARIMA_OK;
    const int64_t nd = N * (int64_t)sizeof(double), ni = N * (int64_t)sizeof(int32_t);
    PASSCHK(f.bind({buf_in(series, strided_bytes(N, ld, T), T > 0), x_block(xreg, (int64_t)n_xcols * T, N, xs),
                    buf_out(coef_out, nd * (1 + n_xcols)), buf_out(rho_out, nd), buf_opt_out(n_iter_out, ni),
                    buf_out(status_out, ni)}));
    PASSCHK(f.overlap());
    PASSCHK(f.begin(stream));
    PASSCHK(co_dev(h, d, rg_src(f, ld, xs), N, max_iter, f.dev<double>(2), f.dev<double>(3), f.dev<int32_t>(4),
                   f.dev<int32_t>(5), f.s()));
    return f.finish();
}

int arima_regarima_co_fit_batch(arima_handle *h, const double *series, int64_t N, int32_t T, const double *xreg,
                                int64_t x_series_stride, int32_t n_xcols, int32_t max_iter, double *coef_out,
                                double *rho_out, int32_t *n_iter_out, int32_t *status_out) {
    return co_body(h, kHostBuffers, series, N, T, T, xreg, x_series_stride, n_xcols, max_iter, coef_out, rho_out,
                   n_iter_out, status_out, nullptr);
}

int arima_regarima_co_fit_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                       const double *d_xreg, int64_t x_series_stride, int32_t n_xcols,
                                       int32_t max_iter, double *d_coef_out, double *d_rho_out,
                                       int32_t *d_n_iter_out, int32_t *d_status_out, void *stream) {
    return co_body(h, kDeviceBuffers, d_series, N, T, ld, d_xreg, x_series_stride, n_xcols, max_iter, d_coef_out,
                   d_rho_out, d_n_iter_out, d_status_out, stream);
}

// ---------------------------------------------------------------------------------------------------------
// ARIMAX.fitModel and ARIMAXModel.forecast (ARIMAX.scala:59-161, :201-256; arima_arimax.hip)
// ---------------------------------------------------------------------------------------------------------
namespace {
struct AxShape {
    int32_t T, k, p, d, q, L, orig, I;
    int64_t num_x() const { return (int64_t)k * L + (orig ? k : 0); }
    int64_t num_coef() const { return 1 + (int64_t)p + q + num_x(); }
};

// argument rules shared by the ARIMAX entry points; x_rows: the rows of a regressor matrix (T for a fit, n_future for
// a forecast); *done: nothing to compute (ARIMA_OK)
int arimax_check(arima_handle *h, const AxShape &a, int64_t N, int64_t ld, int64_t xs, int64_t x_rows, bool *done) {
    *done = false;
    if (N < 0 || a.T < 0 || ld < a.T || x_rows < 0) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    if (a.k < 1) return set_err(h, ARIMA_E_INVALID_ARG, "n_xcols < 1");
    if (a.p < 0 || a.d < 0 || a.q < 0 || a.L < 0) return set_err(h, ARIMA_E_INVALID_ARG, "negative order or lag");
    if (xs != 0 && xs < (int64_t)a.k * x_rows) return set_err(h, ARIMA_E_INVALID_ARG, "x_series_stride below one matrix");
    if (!sts::gen_orders_ok(a.p, a.q)) return set_err(h, ARIMA_E_UNSUPPORTED, "p, q <= 20");
    if (a.d > 16) return set_err(h, ARIMA_E_UNSUPPORTED, "d <= 16");
    if (a.num_coef() > sts::kGenMaxK) return set_err(h, ARIMA_E_UNSUPPORTED, "at most 41 coefficients");
    if ((int64_t)a.k * x_rows > INT32_MAX) return set_err(h, ARIMA_E_UNSUPPORTED, "regressor matrix too large");
    // the kernels index a series' arrays of up to (d + 1) T + n_future values with int
    if (((int64_t)a.d + 2) * a.T + x_rows > INT32_MAX) return set_err(h, ARIMA_E_UNSUPPORTED, "series too long");
    *done = N == 0;
    return ARIMA_OK;
}

// The fit of every series, slice by slice, in the handle's regress workspace. A slice of n series holds, per series:
// the ARX design ((C + 1) R doubles), the flat-differenced regressors (k T; one copy for the whole call when the matrix
// is shared), the differenced series, the ARX and Hannan-Rissanen results and the start point. With user_init only the
// differenced series is needed.
int arimax_fit_dev(arima_handle *h, const AxShape &a, const double *y, int64_t ld, const double *x, int64_t xs, int64_t N,
                   const double *user_init, const sts::FitOut &o, hipStream_t s) {
    const int T = a.T, k = a.k, p = a.p, d = a.d, q = a.q, I = a.I;
    const int nX = (int)a.num_x(), Kp = (int)a.num_coef(), Ka = 1 + p + nX, Kh = std::max(I + p + q, 1);
    const int n = std::max(T - d, 0);
    const int64_t ldn = row_stride(h, n), kT = (int64_t)k * T;
    // the ARX regression always has an intercept (AutoregressionX.fitModel's default)
    const RgDesign dsg = arx_design(T, k, p, a.L, a.orig, 0);
    const int32_t shape = regress_shape_status(dsg);
    const bool start = user_init == nullptr, design = start && shape == ARIMA_ST_OK;
    const int R = design ? dsg.rows() : 0, C = design ? dsg.cols() : 0;
    const int64_t per_series = (design ? (int64_t)(C + 1) * R + (xs ? kT : 0) : 0) + ldn +
                               (start ? (int64_t)Ka + Kh + Kp + 2 : 0);
    int64_t slice_bytes;
    PASSCHK(auto_slice_bytes(h, h->regress_slice_bytes, h->rg_ws.bytes, &slice_bytes));
    const int64_t slice = sts::plan::regress_slice_rows(slice_bytes, per_series), ns = std::min(slice, N);
    // (the differenced rows behind them stay 128-byte aligned)
    const int64_t ws_d = design ? sts::rg_ws_doubles(ns, R, C) : 0, dx_d = design ? round_up(xs ? ns * kT : kT, 16) : 0;
    const int64_t start_d = start ? ns * ((int64_t)Ka + Kh + Kp + 2) : 0;
    RCCHK(h, h->rg_ws.ensure((size_t)(ws_d + dx_d + ns * ldn + start_d + 16) * sizeof(double)), "regression workspace");
    double *ws = h->rg_ws.as<double>(), *dx = ws + ws_d, *dy = dx + dx_d, *arx = dy + ns * ldn, *hr = arx + ns * Ka,
           *init = hr + ns * Kh;
    int32_t *arx_st = reinterpret_cast<int32_t *>(init + ns * Kp), *hr_st = arx_st + ns, *init_st = hr_st + ns;
    // estimateARXCoefficients (:98-102): the column-major matrix differenced as ONE vector of k T values
    if (design && xs == 0) RCCHK(h, sts::launch_difference(x, kT, dx, kT, 1, (int)kT, d, 0, s), "xreg difference");
    for (int64_t f = 0; f < N; f += slice) {
        const int64_t m = std::min(slice, N - f);
        RCCHK(h, sts::launch_difference(y + f * ld, ld, dy, ldn, m, T, d, 1, s), "difference");
        if (start) {
            if (design) {
                if (xs != 0) RCCHK(h, sts::launch_difference(x + f * xs, xs, dx, kT, m, (int)kT, d, 0, s), "xreg difference");
                const RgSrc src{y + f * ld, ld, dx, xs ? kT : 0};
                RCCHK(h, sts::launch_regress_assemble(dsg, src, m, ws, s), "design");
                RCCHK(h, sts::launch_regress_qr(ws, m, R, C, arx, Ka, 0, 0, arx_st, s), "qr");
            } else {
                RCCHK(h, sts::launch_regress_refuse(m, shape, arx_st, arx, Ka, nullptr, 0, s), "regression");
            }
            // estimateMACoefficients (:111-117): the regression runs, and can throw, with q == 0 too
            RCCHK(h, sts::launch_hr_init(dy, ldn, n, m, p, q, I, hr, hr_st, s, std::max(h->hr_grid, 0)), "hr_init");
            RCCHK(h, sts::launch_arimax_splice(arx, arx_st, hr, hr_st, m, p, q, I, nX, init, init_st, s), "start point");
        }
        RCCHK(h, sts::launch_arimax_fit(dy, ldn, n, m, p, q, I, Kp, h->smear, start ? init : user_init + f * Kp,
                                        start ? init_st : nullptr, o.at(f, Kp), s), "arimax fit");
    }
    return ARIMA_OK;
}

// ARIMAXModel.forecast's own shapes: the reference throws for every series alike (tests/arimax_ref.py forecast_check)
int arimax_forecast_check(arima_handle *h, const AxShape &a, int32_t n_future) {
    const int64_t M = std::max(a.p, a.q), R = M + std::max(n_future - a.d, 0);
    if (M == 0) return set_err(h, ARIMA_E_INVALID_ARG, "max(p, q) == 0");
    if (a.T < a.d) return set_err(h, ARIMA_E_INVALID_ARG, "T < d");
    if (R - a.L < 0) return set_err(h, ARIMA_E_INVALID_ARG, "fewer differenced xreg rows than xreg_max_lag");
    if (R - a.L > M + a.T - a.d) return set_err(h, ARIMA_E_INVALID_ARG, "more predictor rows than history");
    return ARIMA_OK;
}

int arimax_forecast_dev(arima_handle *h, const AxShape &a, const double *ts, int64_t ld, const double *x, int64_t xs,
                        int32_t n_future, const double *coef, double *out, int64_t ld_out, int64_t N, hipStream_t s) {
    const int Kp = (int)a.num_coef();
    // the streaming row-tile kernel at the compiled forecast's orders, the workspace kernel above them
    if (!sts::gen_order(a.p, a.q) && a.d <= 8)
        return sts::launch_arimax_forecast_stream(ts, ld, x, xs, a.k, coef, Kp, out, ld_out, N, a.T, a.p, a.d, a.q, a.I,
                                                  a.L, a.orig, n_future, s);
    const int64_t w = sts::arimax_forecast_ws_doubles(a.T, a.p, a.d, a.q, n_future);
    return forecast_slices(h, N, w, "arimax forecast", [&](int64_t f, int64_t m, double *ws) {
        return sts::launch_arimax_forecast(ts + f * ld, ld, x + f * xs, xs, a.k, coef + f * Kp, Kp, out + f * ld_out,
                                           ld_out, m, a.T, a.p, a.d, a.q, a.I, a.L, a.orig, n_future, ws, w, s);
    });
}
}  // namespace

int arima_arimax_num_coef(int32_t n_xcols, int32_t p, int32_t q, int32_t xreg_max_lag, int32_t include_original_xreg) {
    if (n_xcols < 0 || p < 0 || q < 0 || xreg_max_lag < 0) return ARIMA_E_INVALID_ARG;
    const int64_t K = AxShape{0, n_xcols, p, 0, q, xreg_max_lag, include_original_xreg ? 1 : 0, 1}.num_coef();
    return K > INT32_MAX ? ARIMA_E_INVALID_ARG : (int)K;
}

static int arimax_fit_body(arima_handle *h, CallFlavour flavour, const double *series, int64_t N, int64_t ld,
                           const double *xreg, int64_t xs, const AxShape &a, const double *user_init, double *coef_out,
                           double *ll_out, int32_t *status_out, int32_t *n_eval_out, int32_t *n_grad_out,
                           void *stream) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, flavour);
    bool done;
    PASSCHK(arimax_check(h, a, N, ld, xs, a.T, &done));
    if (done) return ARIMA_OK;
    const int64_t nd = N * (int64_t)sizeof(double), ni = N * (int64_t)sizeof(int32_t), coef_bytes = nd * a.num_coef();
    PASSCHK(f.bind({buf_in(series, strided_bytes(N, ld, a.T), a.T > 0), x_block(xreg, (int64_t)a.k * a.T, N, xs),
                    buf_in(user_init, coef_bytes, false), buf_out(coef_out, coef_bytes), buf_out(ll_out, nd),
                    buf_out(status_out, ni), buf_opt_out(n_eval_out, ni), buf_opt_out(n_grad_out, ni)}));
    PASSCHK(f.overlap());
    PASSCHK(f.begin(stream));
    const sts::FitOut o{f.dev<double>(3), f.dev<double>(4), f.dev<int32_t>(5), f.dev<int32_t>(6), f.dev<int32_t>(7),
                        nullptr};
    PASSCHK(arimax_fit_dev(h, a, f.dev<double>(0), ld, f.dev<double>(1), xs, N, f.dev<double>(2), o, f.s()));
    return f.finish();
}

int arima_arimax_fit_batch(arima_handle *h, const double *series, int64_t N, int32_t T, const double *xreg,
                           int64_t x_series_stride, int32_t n_xcols, int32_t p, int32_t d, int32_t q,
                           int32_t xreg_max_lag, int32_t include_original_xreg, int32_t include_intercept,
                           const double *user_init, double *coef_out, double *ll_out, int32_t *status_out,
                           int32_t *n_eval_out, int32_t *n_grad_out) {
    return arimax_fit_body(h, kHostBuffers, series, N, T, xreg, x_series_stride,
                           {T, n_xcols, p, d, q, xreg_max_lag, include_original_xreg ? 1 : 0, include_intercept ? 1 : 0},
                           user_init, coef_out, ll_out, status_out, n_eval_out, n_grad_out, nullptr);
}

int arima_arimax_fit_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                  const double *d_xreg, int64_t x_series_stride, int32_t n_xcols, int32_t p, int32_t d,
                                  int32_t q, int32_t xreg_max_lag, int32_t include_original_xreg,
                                  int32_t include_intercept, const double *d_user_init, double *d_coef_out,
                                  double *d_ll_out, int32_t *d_status_out, int32_t *d_n_eval_out,
                                  int32_t *d_n_grad_out, void *stream) {
    return arimax_fit_body(h, kDeviceBuffers, d_series, N, ld, d_xreg, x_series_stride,
                           {T, n_xcols, p, d, q, xreg_max_lag, include_original_xreg ? 1 : 0, include_intercept ? 1 : 0},
                           d_user_init, d_coef_out, d_ll_out, d_status_out, d_n_eval_out, d_n_grad_out, stream);
}

static int arimax_forecast_body(arima_handle *h, CallFlavour flavour, const double *series, int64_t N, int64_t ld,
                                const double *xreg, int64_t xs, int32_t n_future, const AxShape &a, const double *coef,
                                double *out, int64_t ld_out, void *stream) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, flavour);
    bool done;
    PASSCHK(arimax_check(h, a, N, ld, xs, n_future, &done));
    if (ld_out < a.T) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    PASSCHK(arimax_forecast_check(h, a, n_future));
    if (done || a.T == 0) return ARIMA_OK;
    // (the regressor block is needed also when there is no future row to read)
    PASSCHK(f.bind({buf_in(series, strided_bytes(N, ld, a.T)),
                    buf_in(xreg, x_block(xreg, (int64_t)a.k * n_future, N, xs).bytes),
                    buf_in(coef, N * a.num_coef() * (int64_t)sizeof(double)),
                    buf_out(out, strided_bytes(N, ld_out, a.T))}));
    PASSCHK(f.overlap());
    PASSCHK(f.begin(stream));
    PASSCHK(arimax_forecast_dev(h, a, f.dev<double>(0), ld, f.dev<double>(1), xs, n_future, f.dev<double>(2),
                                f.dev<double>(3), ld_out, N, f.s()));
    return f.finish();
}

int arima_arimax_forecast_batch(arima_handle *h, const double *series, int64_t N, int32_t T, const double *xreg,
                                int64_t x_series_stride, int32_t n_xcols, int32_t n_future, int32_t p, int32_t d,
                                int32_t q, int32_t xreg_max_lag, int32_t include_original_xreg,
                                int32_t include_intercept, const double *coef, double *out) {
    return arimax_forecast_body(h, kHostBuffers, series, N, T, xreg, x_series_stride, n_future,
                                {T, n_xcols, p, d, q, xreg_max_lag, include_original_xreg ? 1 : 0,
                                 include_intercept ? 1 : 0}, coef, out, T, nullptr);
}

int arima_arimax_forecast_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                       const double *d_xreg, int64_t x_series_stride, int32_t n_xcols,
                                       int32_t n_future, int32_t p, int32_t d, int32_t q, int32_t xreg_max_lag,
                                       int32_t include_original_xreg, int32_t include_intercept, const double *d_coef,
                                       double *d_out, int64_t ld_out, void *stream) {
    return arimax_forecast_body(h, kDeviceBuffers, d_series, N, ld, d_xreg, x_series_stride, n_future,
                                {T, n_xcols, p, d, q, xreg_max_lag, include_original_xreg ? 1 : 0,
                                 include_intercept ? 1 : 0}, d_coef, d_out, ld_out, stream);
}


// ---------------------------------------------------------------------------------------------------------
// order search over (d, p, q, intercept) — SURVEY.md 8(f) row 2 (config C5)
// ---------------------------------------------------------------------------------------------------------
// Stream s waits for everything the first L search lanes have been given so far. The entry points join every lane,
// also after an error part-way through the grid: later calls then wait for the lanes' reads of the search
// workspaces through h->ev_done.
static void join_lanes(arima_handle *h, hipStream_t s, int L = kMaxSearchLanes) {
    for (int j = 0; j < L; ++j) {
        SearchLane &ln = h->lanes[j];
        if (!ln.stream) continue;
        if (hipEventRecord(ln.ev_fit, ln.stream) == hipSuccess) hipStreamWaitEvent(s, ln.ev_fit, 0);
    }
}

static int order_search_locked(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                               int32_t max_p, int32_t max_d, int32_t max_q, int32_t intercept_mode, int32_t method,
                               int32_t *d_order, double *d_coef, double *d_aic, int64_t *n_fits, hipStream_t s) {
    if (max_p < 0 || max_q < 0 || max_d < 0 || intercept_mode < 0 || intercept_mode > 2)
        return set_err(h, ARIMA_E_INVALID_ARG, "bad search bounds");
    if (max_p > 5 || max_q > 5 || max_d > kMaxD) return set_err(h, ARIMA_E_UNSUPPORTED, "p, q <= 5, d <= 16");
    if (N < 0 || T < 0 || ld < T || !d_order || !d_coef || !d_aic) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    h->stats_from = StatsFrom::kNone;
    h->stats = arima_fit_stats{};
    if (N == 0) return ARIMA_OK;
    HIPCHK(h, hipSetDevice(h->device));
    // Differenced copies: one per d, all computed up front, so the lanes run through the d boundaries without
    // draining -- when they fit in HBM next to the lanes' workspaces; otherwise one shared copy, rewritten for each
    // d once every fit of the previous d has finished (max_d up to 16 would not fit).
    size_t diff_bytes = 0;
    for (int d = 0; d <= max_d; ++d) diff_bytes += (size_t)N * row_stride(h, T - d) * sizeof(double);
    const size_t lane_bytes = (size_t)N * (11 * 8 * 2 + 8 + 4 * 4 + 1 + 8 + 16 + 88) + sts::kExpressRingBytes +
                              sts::kExpressReadyBytes;
    size_t free_b = 0, total_b = 0;
    HIPCHK(h, hipMemGetInfo(&free_b, &total_b));
    size_t held = 0;                               // what this handle's search workspaces already hold
    for (int d = 0; d <= kMaxD; ++d) held += h->os_diff[d].bytes;
    const bool per_d = diff_bytes + (size_t)h->search_lanes * lane_bytes <= (free_b + held) / 10 * 9;
    // Lanes: as many of the configured as their workspaces allow (at least one)
    int L = 0;
    for (int j = 0; j < h->search_lanes; ++j) {
        SearchLane &ln = h->lanes[j];
        if (!ln.stream) {
            HIPCHK(h, hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
            HIPCHK(h, hipEventCreateWithFlags(&ln.ev_fit, hipEventDisableTiming));
            HIPCHK(h, hipEventCreateWithFlags(&ln.ev_sel, hipEventDisableTiming));
        }
        // every workspace at its largest size before anything is enqueued: a growing DevBuf frees (hipFree
        // synchronises the device) and would serialise the host loop below with the fits already in flight
        int rc = ln.ws.reserve(N, 11);
        if (rc == ARIMA_OK) rc = ln.coef.ensure((size_t)N * 11 * sizeof(double));
        if (rc == ARIMA_OK) rc = ln.ll.ensure((size_t)N * sizeof(double));
        for (DevBuf *b : {&ln.status, &ln.neval, &ln.ngrad})
            if (rc == ARIMA_OK) rc = b->ensure((size_t)N * sizeof(int32_t));
        if (rc == ARIMA_OK) rc = ln.flags.ensure((size_t)N);
        if (rc == ARIMA_OK) rc = ln.best_aic.ensure((size_t)N * sizeof(double));
        if (rc == ARIMA_OK) rc = ln.best_order.ensure((size_t)N * 4 * sizeof(int32_t));
        if (rc == ARIMA_OK) rc = ln.best_coef.ensure((size_t)N * 11 * sizeof(double));
        if (rc == ARIMA_OK) rc = ln.acc.ensure((kCtlWords + 1 + kExtWords) * sizeof(unsigned long long));
        if (rc != ARIMA_OK) {
            if (j == 0) return set_err(h, rc, "order search workspace");
            break;                                 // fewer lanes instead of failing the call
        }
        L = j + 1;
    }
    if (per_d) {
        for (int d = 0; d <= max_d; ++d)
            RCCHK(h, h->os_diff[d].ensure((size_t)N * row_stride(h, T - d) * sizeof(double)), "workspace");
    } else {
        RCCHK(h, h->os_diff[0].ensure((size_t)N * row_stride(h, T) * sizeof(double)), "workspace");
    }
    HIPCHK(h, hipEventRecord(h->ev[0], s));
    auto diff_into = [&](int d, DevBuf &buf) -> int {
        const int n = std::max(T - d, 0);
        const int64_t ldn = row_stride(h, n);
        if (!h->ev_diff[d]) HIPCHK(h, hipEventCreateWithFlags(&h->ev_diff[d], hipEventDisableTiming));
        RCCHK(h, sts::launch_difference(d_series, ld, buf.as<double>(), ldn, N, T, d, 1, s), "difference");
        HIPCHK(h, hipEventRecord(h->ev_diff[d], s));
        return ARIMA_OK;
    };
    if (per_d)                                     // differencesOfOrderD once per d (ARIMA.scala:88)
        for (int d = 0; d <= max_d; ++d) RCCHK(h, diff_into(d, h->os_diff[d]), "difference");
    // Every lane keeps its own best candidate per series, and candidates compare by (approxAIC, grid position), so
    // the result does not depend on the order the grid points finish in: each lane runs its grid points back to back
    // without waiting for the others (a lane's long fit no longer holds the other lanes' next fits). With one
    // differenced copy per d the grid points go to the lanes by estimated cost, longest first (LPT); with the shared
    // copy they keep the (d, p, q, intercept) order and the lanes join before the copy is rewritten.
    for (int j = 0; j < L; ++j) {
        SearchLane &ln = h->lanes[j];
        HIPCHK(h, hipStreamWaitEvent(ln.stream, h->ev[0], 0));
        RCCHK(h, sts::launch_search_init(ln.best_aic.as<double>(), ln.best_order.as<int32_t>(),
                                         ln.best_coef.as<double>(), N, ln.stream), "search_init");
        HIPCHK(h, hipMemsetAsync(ln.acc.ptr, 0, (kCtlWords + 1 + kExtWords) * sizeof(unsigned long long), ln.stream));
    }
    const int i_lo = intercept_mode == 1 ? 1 : 0, i_hi = intercept_mode == 0 ? 0 : 1;
    struct GridPoint { int d, p, q, I; double cost; };
    std::vector<GridPoint> grid;
    for (int d = 0; d <= max_d; ++d)
        for (int p = 0; p <= max_p; ++p)
            for (int q = 0; q <= max_q; ++q)
                for (int I = i_lo; I <= i_hi; ++I)
                    // ms per 65 536 series in profiles/r03/b_c3_c5/grid_65536.jsonl follow (1+p)(1+q) (corr. 0.8);
                    // AR-only fits (q = 0) are a single OLS
                    grid.push_back({d, p, q, I, q == 0 ? 0.1 : (double)(1 + p) * (1 + q)});
    std::vector<std::vector<int>> plan(L);
    if (per_d) {
        std::vector<int> idx(grid.size());
        for (size_t g = 0; g < grid.size(); ++g) idx[g] = (int)g;
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return grid[a].cost > grid[b].cost; });
        std::vector<double> load(L, 0.0);
        for (int g : idx) {
            const int j = (int)(std::min_element(load.begin(), load.end()) - load.begin());
            plan[j].push_back(g);
            load[j] += grid[g].cost;
        }
    } else {
        for (size_t g = 0; g < grid.size(); ++g) plan[g % L].push_back((int)g);
    }
    int64_t fits = 0;
    FitOpts lane_opt;
    lane_opt.shared_gpu = L > 1;
    if (L > 1) lane_opt.express_cus = h->search_express_blocks;
    lane_opt.search = true;
    // the shared differenced copy: the fits of one d at a time (plan order is d-major on every lane)
    for (int dd = 0; dd <= (per_d ? 0 : max_d); ++dd) {
        if (!per_d) {
            if (dd > 0) join_lanes(h, s, L);        // every fit of d - 1 has read the copy
            RCCHK(h, diff_into(dd, h->os_diff[0]), "difference");
        }
        for (int j = 0; j < L; ++j) {
            SearchLane &ln = h->lanes[j];
            for (int g : plan[j]) {
                const GridPoint &gp = grid[g];
                if (!per_d && gp.d != dd) continue;
                const int d = gp.d, p = gp.p, q = gp.q, I = gp.I;
                const int n = std::max(T - d, 0);
                const int64_t ldn = row_stride(h, n);
                DevBuf &dbuf = per_d ? h->os_diff[d] : h->os_diff[0];
                HIPCHK(h, hipStreamWaitEvent(ln.stream, h->ev_diff[d], 0));
                // ARIMA(0,d,0) without intercept has no parameters: the reference throws (NoDataException);
                // fit_kernels reports it per series and the select step skips it.
                int64_t gridb = 0, xb = 0;
                RCCHK(h, fit_kernels(h, ln.ws, dbuf.as<double>(), ldn, n, N, p, q, I, method, nullptr, ln.out(),
                                     ln.stream, &gridb, &xb, lane_opt), "fit");
                if (gridb > 0) {
                    h->last_grid = gridb;
                    h->last_express = xb;
                }
                hipLaunchKernelGGL(k_search_acc, dim3(1), dim3(64), 0, ln.stream, ln.ws.ctl.as<unsigned long long>(),
                                   ln.acc.as<unsigned long long>(), N, n, p, q, I,
                                   (p > 0 && q == 0) || method != ARIMA_METHOD_CSS_CGD || I + p + q == 0 ? 0 : 1);
                HIPCHK(h, hipGetLastError());
                // a fit whose kernel recorded a watchdog fault contributes nothing (its outputs are incomplete) and
                // the fault reaches the caller through the handle's sticky record (arima_synchronize)
                RCCHK(h, sts::launch_search_select(ln.coef.as<double>(), ln.ll.as<double>(), ln.status.as<int32_t>(),
                                                   ln.flags.as<uint8_t>(), N, p, d, q, I,
                                                   ln.ws.ctl.as<unsigned long long>(), ln.best_aic.as<double>(),
                                                   ln.best_order.as<int32_t>(), ln.best_coef.as<double>(),
                                                   ln.stream),
                      "search_select");
                ++fits;
            }
        }
    }
    join_lanes(h, s, L);
    sts::SearchBests bests{};
    for (int j = 0; j < L; ++j) {
        bests.aic[j] = h->lanes[j].best_aic.as<double>();
        bests.order[j] = h->lanes[j].best_order.as<int32_t>();
        bests.coef[j] = h->lanes[j].best_coef.as<double>();
    }
    RCCHK(h, sts::launch_search_merge(bests, L, N, d_aic, d_order, d_coef, s), "search_merge");
    HIPCHK(h, hipEventRecord(h->ev[3], s));
    for (int j = 0; j < L; ++j) {                  // the lanes' counter sums, read by arima_get_last_stats
        HIPCHK(h, hipMemcpyAsync(h->search_acc_host + (size_t)j * (kCtlWords + 1), h->lanes[j].acc.ptr,
                                 (kCtlWords + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(h->search_acc_host + (size_t)kMaxSearchLanes * (kCtlWords + 1) + (size_t)j * kExtWords,
                                 h->lanes[j].acc.as<unsigned long long>() + kCtlWords + 1,
                                 kExtWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(h, hipEventRecord(h->ev[4], s));
    h->stats_from = StatsFrom::kSearch;
    h->search_lanes_used = L;
    h->search_n = N;
    h->search_fits = fits;
    if (n_fits) *n_fits = fits;
    return ARIMA_OK;
}

// Blocking entry points: the fault record covers the lanes' fit kernels (a dropped series must not
// pass as a candidate, and the call reports ARIMA_E_DEVICE).
static int take_fault(arima_handle *h) {
    unsigned long long f[6] = {};
    unsigned long long *rec = h->dev_fault.as<unsigned long long>();
    hipLaunchKernelGGL(k_fault_take, dim3(1), dim3(64), 0, h->stream, rec);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(f, rec + 8, sizeof f, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return f[0] == 0 ? ARIMA_OK : report_fault(h, f);
}

int arima_order_search_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T,
                                    int64_t ld, int32_t max_p, int32_t max_d, int32_t max_q,
                                    int32_t intercept_mode, int32_t method, int32_t *d_order_out,
                                    double *d_coef_out, double *d_aic_out, void *stream) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, kDeviceBuffers);
    PASSCHK(f.begin(stream));
    const int rc = order_search_locked(h, d_series, n_series, T, ld, max_p, max_d, max_q, intercept_mode, method,
                                       d_order_out, d_coef_out, d_aic_out, nullptr, f.s());
    join_lanes(h, f.s());
    return f.finish(rc);
}

int arima_order_search_batch(arima_handle *h, const double *series, int64_t N, int32_t T, int32_t max_p,
                             int32_t max_d, int32_t max_q, int32_t intercept_mode, int32_t method,
                             int32_t *order_out, double *coef_out, double *aic_out) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, kHostBuffers);
    if (N < 0 || T < 0) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    if (N == 0) return ARIMA_OK;
    if (!series || !order_out || !coef_out || !aic_out) return set_err(h, ARIMA_E_INVALID_ARG, "null buffer");
    PASSCHK(f.begin());
    const size_t nd = (size_t)N * sizeof(double);
    PASSCHK(f.stage({buf_in(series, nd * T), buf_out(order_out, (size_t)N * 4 * sizeof(int32_t)),
                     buf_out(coef_out, 11 * nd), buf_out(aic_out, nd)}));
    int rc = order_search_locked(h, f.dev<double>(0), N, T, T, max_p, max_d, max_q, intercept_mode, method,
                                 f.dev<int32_t>(1), f.dev<double>(2), f.dev<double>(3), nullptr, f.s());
    join_lanes(h, f.s());
    rc = f.finish(rc);
    if (rc != ARIMA_OK) return rc;
    return take_fault(h);
}

// ---------------------------------------------------------------------------------------------------------
// ARIMA.autoFit over a batch (ARIMA.scala:280-375; arima_autofit.hip has the kernels and the quirks they restate)
// ---------------------------------------------------------------------------------------------------------
// Host loop: (1) the KPSS search over d = 0..max_d (rows of undecided series differenced at d into af_rows, then the
// test; decided rows keep their d); (2) rounds of the stepwise walk: k_af_plan appends every walking series'
// candidates to per-(p, q, intercept) lists, the host reads the list sizes (one small copy per round), and every
// non-empty list is gathered and fitted as one batch (fit_kernels: AR-only OLS or HR init + k_cg_fit) on the fit
// contexts' streams, several orders at once; k_af_update then picks each series' new incumbent and neighbourhood.
// The walk ends when no series has candidates left (at most max_p + 2 rounds after the first).
constexpr int kAfContexts = 4;                     // fit contexts the orders of one round rotate over

// One slice of the batch (every workspace sized for N series of length T). max_p <= sts::kAfMaxP.
static int autofit_slice(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld, int32_t max_p,
                         int32_t max_d, int32_t max_q, int32_t *d_order, double *d_coef, double *d_aic,
                         int32_t *d_status, int32_t *d_nfits, hipStream_t s, int64_t *fits_out) {
    const int ncombos = sts::af_combos(max_p);
    const int64_t ldT = row_stride(h, T);
    const int64_t rows_max = N * sts::kAfMaxCand;  // candidate fits of one round, at most
    RCCHK(h, h->af_rows.ensure((size_t)N * ldT * sizeof(double)), "autofit workspace");
    RCCHK(h, h->af_dsel.ensure((size_t)N * sizeof(int32_t)), "autofit workspace");
    RCCHK(h, h->af_state.ensure((size_t)N * sizeof(sts::AfSeries)), "autofit workspace");
    RCCHK(h, h->af_best.ensure((size_t)N * 11 * sizeof(double)), "autofit workspace");
    RCCHK(h, h->af_counts.ensure(sts::kAfCombosMax * sizeof(unsigned)), "autofit workspace");
    RCCHK(h, h->af_off.ensure(sts::kAfCombosMax * sizeof(int64_t)), "autofit workspace");
    RCCHK(h, h->af_lists.ensure((size_t)ncombos * N * sizeof(int32_t)), "autofit workspace");
    RCCHK(h, h->af_coef.ensure((size_t)rows_max * 11 * sizeof(double)), "autofit workspace");
    RCCHK(h, h->af_ll.ensure((size_t)rows_max * sizeof(double)), "autofit workspace");
    RCCHK(h, h->af_status.ensure((size_t)rows_max * sizeof(int32_t)), "autofit workspace");
    RCCHK(h, h->af_flags.ensure((size_t)rows_max), "autofit workspace");
    RCCHK(h, h->af_init.ensure((size_t)rows_max * 11 * sizeof(double)), "autofit workspace");
    RCCHK(h, h->af_hrst.ensure((size_t)rows_max * sizeof(int32_t)), "autofit workspace");
    RCCHK(h, h->af_rlist.ensure((size_t)sts::kBqRefitBuckets * rows_max * sizeof(int32_t)), "autofit workspace");
    RCCHK(h, h->af_rcount.ensure(sts::kBqRefitBuckets * sizeof(unsigned)), "autofit workspace");
    if (!h->af_host && hipHostMalloc((void **)&h->af_host, (2 * sts::kAfCombosMax + sts::kBqRefitBuckets) * sizeof(int64_t),
                                     0) != hipSuccess)
        return set_err(h, ARIMA_E_OOM, "pinned");
    if (!h->ev_af) HIPCHK(h, hipEventCreateWithFlags(&h->ev_af, hipEventDisableTiming));
    const int P = std::min(kAfContexts, kMaxPipeline);
    // every context's gather buffer and fit workspace at full size
    RCCHK(h, reserve_fit_ws(h, P, N, ldT, 11), "autofit workspace");
    for (int j = 0; j < P; ++j)
        if (h->fctx[j].has_done) HIPCHK(h, hipStreamWaitEvent(s, h->fctx[j].ev_done, 0));
    // the round's results, one row per candidate fit (coefficient rows of 11 doubles; no evaluation counts)
    const FitOut af{h->af_coef.as<double>(), h->af_ll.as<double>(), h->af_status.as<int32_t>(), nullptr, nullptr,
                    h->af_flags.as<uint8_t>()};
    FitOpts af_opt;
    af_opt.shared_gpu = P > 1;
    // (1) d: the first of 0..max_d whose differencesOfOrderD(ts, d) passes kpsstest(_, "c") (ARIMA.scala:287-297)
    const int32_t kpss_st = kpss_shape_status(T);
    int32_t *dsel = h->af_dsel.as<int32_t>();
    HIPCHK(h, hipMemsetAsync(dsel, 0xff, (size_t)N * sizeof(int32_t), s));
    if (kpss_st == ARIMA_ST_OK) {
        for (int d = 0; d <= max_d; ++d) {
            RCCHK(h, sts::launch_difference_sel(d_series, ld, h->af_rows.as<double>(), ldT, N, T, dsel, d, s),
                  "difference");
            RCCHK(h, sts::launch_kpss_c(h->af_rows.as<double>(), ldT, T, N, d, dsel, nullptr, s), "kpss");
        }
    }
    // (2) the stepwise walk (findBestARMAModel, :310-375) on each series' differenced row
    sts::AfSeries *st = h->af_state.as<sts::AfSeries>();
    RCCHK(h, sts::launch_af_init(N, dsel, st, kpss_st, s), "autofit init");
    int64_t fits = 0;
    for (int round = 0; kpss_st == ARIMA_ST_OK; ++round) {
        HIPCHK(h, hipMemsetAsync(h->af_counts.ptr, 0, ncombos * sizeof(unsigned), s));
        RCCHK(h, sts::launch_af_plan(N, st, h->af_counts.as<unsigned>(), h->af_lists.as<int32_t>(), s), "autofit plan");
        unsigned counts[sts::kAfCombosMax];
        HIPCHK(h, hipMemcpyAsync(h->af_host, h->af_counts.ptr, ncombos * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        memcpy(counts, h->af_host, ncombos * sizeof(unsigned));
        int64_t *off = h->af_host + sts::kAfCombosMax;
        int64_t total = 0;
        for (int cb = 0; cb < ncombos; ++cb) {
            off[cb] = total;
            total += counts[cb];
        }
        if (total == 0) break;
        fits += total;
        HIPCHK(h, hipMemcpyAsync(h->af_off.ptr, off, ncombos * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIPCHK(h, hipEventRecord(h->ev_af, s));
        // the round's orders, largest list first, over the fit contexts (several orders fit at once)
        int order[sts::kAfCombosMax];
        for (int cb = 0; cb < ncombos; ++cb) order[cb] = cb;
        std::stable_sort(order, order + ncombos, [&](int a, int b) { return counts[a] > counts[b]; });
        int used = 0;
        for (int oi = 0; oi < ncombos && counts[order[oi]] > 0; ++oi) {
            const int cb = order[oi];
            const int p = (cb / 2) / 3, q = (cb / 2) % 3, I = cb % 2;
            const int64_t cnt = counts[cb];
            FitCtx &c = h->fctx[used % P];
            HIPCHK(h, hipStreamWaitEvent(c.stream, h->ev_af, 0));
            RCCHK(h, sts::launch_gather_rows(h->af_rows.as<double>(), ldT, h->af_lists.as<int32_t>() + (int64_t)cb * N,
                                             cnt, T, c.diff.as<double>(), c.stream), "gather");
            int64_t gridb = 0, xb = 0;
            // fitModel(p, 0, q, diffedTs, intercept, "css-cgd") (:316); rows of order cb from off[cb] (coef stride k);
            // p > 5: the runtime-order path (fit_kernels dispatches it)
            RCCHK(h, fit_kernels(h, c.ws, c.diff.as<double>(), ldT, T, cnt, p, q, I, ARIMA_METHOD_CSS_CGD, nullptr,
                                 af.at(off[cb], 11), c.stream, &gridb, &xb, af_opt), "fit");
            // the Hannan-Rissanen inits and their status, kept for the round's css-bobyqa retries (below)
            const int k = p + q + I;
            if (!(p > 0 && q == 0) && k > 0) {
                HIPCHK(h, hipMemcpyAsync(h->af_init.as<double>() + off[cb] * 11, c.ws.init.ptr,
                                         (size_t)cnt * k * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
            }
            if (!(p > 0 && q == 0))
                HIPCHK(h, hipMemcpyAsync(h->af_hrst.as<int32_t>() + off[cb], c.ws.hr_status.ptr,
                                         (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToDevice, c.stream));
            HIPCHK(h, end_fit(c, c.stream));
            ++used;
        }
        for (int j = 0; j < std::min(used, P); ++j) HIPCHK(h, hipStreamWaitEvent(s, h->fctx[j].ev_done, 0));
        // fitTryBothStrategies (:315-319): every row of the round whose css-cgd fit threw in the optimizer, refitted
        // with css-bobyqa from the same Hannan-Rissanen init, in place. The rows are listed per dimension k, the host
        // reads the counts back, and each dimension present runs as one kernel sized by its count (one workgroup per
        // retry, not per candidate row), the dimensions on different streams so they run together
        RCCHK(h, sts::launch_bobyqa_refit_list(h->af_off.as<int64_t>(), ncombos, total, h->af_status.as<int32_t>(),
                                               h->af_rlist.as<int32_t>(), rows_max, h->af_rcount.as<unsigned>(), s),
              "bobyqa list");
        HIPCHK(h, hipMemcpyAsync(h->af_host + 2 * sts::kAfCombosMax, h->af_rcount.ptr,
                                 sts::kBqRefitBuckets * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        unsigned retries[sts::kBqRefitBuckets];
        memcpy(retries, h->af_host + 2 * sts::kAfCombosMax, sizeof retries);
        HIPCHK(h, hipEventRecord(h->ev_af, s));
        int launched = 0;
        for (int k = 2; k < sts::kBqRefitBuckets; ++k) {
            if (retries[k] == 0) continue;
            FitCtx &c = h->fctx[launched % P];
            HIPCHK(h, hipStreamWaitEvent(c.stream, h->ev_af, 0));
            RCCHK(h, sts::launch_bobyqa_refit_dim(k, h->af_rows.as<double>(), ldT, T, h->af_lists.as<int32_t>(), N,
                                                  h->af_off.as<int64_t>(), ncombos, 11,
                                                  h->af_rlist.as<int32_t>() + (int64_t)k * rows_max,
                                                  h->af_rcount.as<unsigned>(), (int64_t)retries[k],
                                                  h->af_init.as<double>(), h->af_hrst.as<int32_t>(), af,
                                                  h->bobyqa_wave != 0, c.stream), "bobyqa refit");
            HIPCHK(h, end_fit(c, c.stream));
            ++launched;
        }
        for (int j = 0; j < std::min(launched, P); ++j) HIPCHK(h, hipStreamWaitEvent(s, h->fctx[j].ev_done, 0));
        RCCHK(h, sts::launch_af_update(N, st, h->af_off.as<int64_t>(), h->af_coef.as<double>(), h->af_ll.as<double>(),
                                       h->af_status.as<int32_t>(), h->af_flags.as<uint8_t>(), h->af_best.as<double>(),
                                       max_p, max_q, s), "autofit update");
        if (round > 64) return set_err(h, ARIMA_E_DEVICE, "autofit: the walk did not end");
    }
    RCCHK(h, sts::launch_af_finish(N, st, h->af_best.as<double>(), d_order, d_coef, d_aic, d_status, d_nfits, s),
          "autofit finish");
    if (fits_out) *fits_out = fits;
    return ARIMA_OK;
}

// ARIMA.autoFit over the batch in slices whose workspaces fit the free HBM (the per-call footprint is ~5x
// the input -- the differenced rows plus one gather buffer per fit context -- so a large batch is cut instead of
// failing with ARIMA_E_OOM); option "autofit_slice" fixes the slice (series), 0 = from free HBM.
static int autofit_locked(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld, int32_t max_p,
                          int32_t max_d, int32_t max_q, int32_t *d_order, double *d_coef, double *d_aic,
                          int32_t *d_status, int32_t *d_nfits, hipStream_t s, int64_t *fits_out) {
    if (max_p < 0 || max_q < 0 || max_d < 0) return set_err(h, ARIMA_E_INVALID_ARG, "bad autofit bounds");
    if (max_p > sts::kAfMaxP || max_d > kMaxD)
        return set_err(h, ARIMA_E_UNSUPPORTED, "autofit: max_p <= 8 (css-bobyqa retries of <= 11 parameters), d <= 16");
    if (N < 0 || T < 0 || ld < T || (N > 0 && (!d_series || !d_order || !d_coef || !d_aic || !d_status)))
        return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    h->stats = arima_fit_stats{};
    h->stats_from = StatsFrom::kNone;
    if (N == 0) return ARIMA_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t ldT = row_stride(h, T);
    int64_t slice = h->autofit_slice;
    if (slice <= 0) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(h, hipMemGetInfo(&free_b, &total_b));
        size_t held = h->af_rows.bytes;            // workspaces this call reuses
        for (int j = 0; j < kAfContexts; ++j) held += h->fctx[j].diff.bytes;
        const int64_t per = (int64_t)(1 + kAfContexts) * ldT * 8 + sts::kAfMaxCand * (11 * 16 + 16) +
                            (int64_t)sts::kAfCombosMax * 4 + 256;
        slice = std::max<int64_t>(4096, (int64_t)((free_b + held) / 10 * 6) / per);
    }
    HIPCHK(h, hipEventRecord(h->ev[0], s));
    int64_t fits = 0;
    for (int64_t f = 0; f < N; f += slice) {
        const int64_t n = std::min(slice, N - f);
        int64_t fs = 0;
        RCCHK(h, autofit_slice(h, d_series + f * ld, n, T, ld, max_p, max_d, max_q, d_order + f * 4, d_coef + f * 11,
                               d_aic + f, d_status + f, d_nfits ? d_nfits + f : nullptr, s, &fs), "autofit");
        fits += fs;
    }
    HIPCHK(h, hipEventRecord(h->ev[3], s));
    h->stats.n_series = fits;
    if (fits_out) *fits_out = fits;
    return ARIMA_OK;
}

int arima_autofit_batch_device(arima_handle *h, const double *d_series, int64_t n_series, int32_t T, int64_t ld,
                               int32_t max_p, int32_t max_d, int32_t max_q, int32_t *d_order_out,
                               double *d_coef_out, double *d_aic_out, int32_t *d_status_out, int32_t *d_n_fits_out,
                               void *stream) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, kDeviceBuffers);
    PASSCHK(f.begin(stream));                    // the device is selected before any stream work
    int rc = autofit_locked(h, d_series, n_series, T, ld, max_p, max_d, max_q, d_order_out, d_coef_out, d_aic_out,
                            d_status_out, d_n_fits_out, f.s(), nullptr);
    rc = f.finish(rc);
    // the walk synchronised with the device once per round, so its fits have finished: a watchdog fault that one of
    // them recorded is reported by this call, not by a later unrelated one
    if (rc != ARIMA_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(f.s()));
    return take_fault(h);
}

int arima_autofit_batch(arima_handle *h, const double *series, int64_t N, int32_t T, int32_t max_p, int32_t max_d,
                        int32_t max_q, int32_t *order_out, double *coef_out, double *aic_out, int32_t *status_out,
                        int32_t *n_fits_out) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, kHostBuffers);
    if (N < 0 || T < 0) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    if (N == 0) return ARIMA_OK;
    if (!series || !order_out || !coef_out || !aic_out || !status_out) return set_err(h, ARIMA_E_INVALID_ARG, "null buffer");
    PASSCHK(f.begin());
    const size_t ni = (size_t)N * sizeof(int32_t), nd = (size_t)N * sizeof(double);
    PASSCHK(f.stage({buf_in(series, nd * T), buf_out(order_out, 4 * ni), buf_out(coef_out, 11 * nd),
                     buf_out(aic_out, nd), buf_out(status_out, ni), buf_opt_out(n_fits_out, ni)}));
    int rc = autofit_locked(h, f.dev<double>(0), N, T, T, max_p, max_d, max_q, f.dev<int32_t>(1), f.dev<double>(2),
                            f.dev<double>(3), f.dev<int32_t>(4), f.dev<int32_t>(5), f.s(), nullptr);
    rc = f.finish(rc);
    if (rc != ARIMA_OK) return rc;
    return take_fault(h);
}

int arima_kpss_batch(arima_handle *h, const double *series, int64_t N, int32_t T, double *stat_out, int32_t *status_out) {
    if (!h || N < 0 || T < 0) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, kHostBuffers);
    if (N == 0) return ARIMA_OK;
    if (!series || !stat_out || !status_out) return set_err(h, ARIMA_E_INVALID_ARG, "null buffer");
    const int32_t st = kpss_shape_status(T);
    PASSCHK(f.begin());
    if (st == ARIMA_ST_OK) {
        int64_t ld = 0;
        RCCHK(h, upload_padded(h, series, N, T, &ld, f.s()), "upload");
        PASSCHK(f.stage({buf_out(stat_out, (size_t)N * sizeof(double))}));
        RCCHK(h, sts::launch_kpss_c(h->diff.as<double>(), ld, T, N, 0, nullptr, f.dev<double>(0), f.s()), "kpss");
    }
    PASSCHK(f.finish());
    for (int64_t i = 0; i < N; ++i) {
        status_out[i] = st;
        if (st != ARIMA_ST_OK) stat_out[i] = NAN;
    }
    return ARIMA_OK;
}

int arima_sample_batch_device(arima_handle *h, double *d_series, int64_t N, int32_t T, int64_t ld, int32_t p,
                              int32_t d, int32_t q, int32_t I, const double *base_coef, double jitter,
                              uint64_t seed, int64_t first_series, void *stream) {
    if (!h || !base_coef || N < 0 || T < 0 || ld < T) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, kDeviceBuffers);
    RCCHK(h, check_orders(h, p, d, q, I), "orders");
    PASSCHK(f.begin(stream));
    RCCHK(h, sts::launch_sample(d_series, ld, N, T, p, d, q, I, base_coef, jitter, seed, first_series, f.s()),
          "sample");
    return f.finish();
}

// ---------------------------------------------------------------------------------------------------------
// the small models: EWMA, GARCH(1,1) and ARGARCH (arima_models.hip) -- fits, objective / gradient, the TimeSeriesModel
// pairs (ARModel's too) and the sample recursions
// ---------------------------------------------------------------------------------------------------------
namespace {
int md_fit_launch(arima_handle *h, int model, const double *rows, int64_t ld, int64_t N, int T, double *coef,
                  double *obj, int32_t *status, int32_t *n_eval, int32_t *n_grad, hipStream_t s) {
    RCCHK(h, h->md_ctl.ensure(sts::kModelCtlWords * sizeof(unsigned long long)), "counters");
    HIPCHK(h, hipMemsetAsync(h->md_ctl.ptr, 0, sts::kModelCtlWords * sizeof(unsigned long long), s));
    const double *aux = nullptr;
    const int32_t *aux_status = nullptr;
    if (model == sts::kModelArGarch) {
        // ARGARCH.fitModel's first stage, Autoregression.fitModel(ts): the kernel arima_fit_batch(1, 0, 0, intercept)
        // runs, into an N x 2 workspace. The GARCH stage reads (c, phi) from it and forms the residuals in its passes.
        RCCHK(h, h->md_ar.ensure((size_t)N * (3 * sizeof(double) + sizeof(int32_t))), "AR workspace");
        double *ar_coef = h->md_ar.as<double>(), *ar_ll = ar_coef + 2 * N;
        int32_t *ar_status = reinterpret_cast<int32_t *>(ar_ll + N);
        RCCHK(h, sts::launch_ar_fit(rows, ld, T, N, 1, 1, sts::FitOut{ar_coef, ar_ll, ar_status, nullptr, nullptr, nullptr},
                                    s), "ar fit");
        aux = ar_coef;
        aux_status = ar_status;
    }
    RCCHK(h, sts::launch_model_fit(model, rows, ld, N, T, coef, obj, status, n_eval, n_grad,
                                   h->md_ctl.as<unsigned long long>(), s, aux, aux_status), "model fit");
    h->md_last_n = N;
    return ARIMA_OK;
}

int md_fit_body(arima_handle *h, CallFlavour flavour, int model, const double *series, int64_t N, int32_t T, int64_t ld,
                double *coef_out, double *obj_out, int32_t *status_out, int32_t *n_eval_out, int32_t *n_grad_out,
                void *stream) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, flavour);
    if (N < 0 || T < 1 || ld < T) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    if (N == 0) return ARIMA_OK;
    const int64_t nd = N * (int64_t)sizeof(double), ni = N * (int64_t)sizeof(int32_t);
    PASSCHK(f.bind({buf_in(series, strided_bytes(N, ld, T)), buf_out(coef_out, nd * sts::model_num_params(model)),
                    buf_out(obj_out, nd), buf_out(status_out, ni), buf_opt_out(n_eval_out, ni),
                    buf_opt_out(n_grad_out, ni)}));
    RCCHK(h, f.overlap(), "overlap");
    PASSCHK(f.begin(stream));
    RCCHK(h, md_fit_launch(h, model, f.dev<double>(0), ld, N, T, f.dev<double>(1), f.dev<double>(2), f.dev<int32_t>(3),
                           f.dev<int32_t>(4), f.dev<int32_t>(5), f.s()), "fit");
    return f.finish();
}

// objective (want_grad == 0: out N) or gradient (out N x K) at params (N x K), host buffers
int md_eval_host(arima_handle *h, int model, const double *series, int64_t N, int32_t T, const double *params,
                 double *out, int want_grad) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, kHostBuffers);
    if (N < 0 || T < 1) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    if (N == 0) return ARIMA_OK;
    const int K = sts::model_num_params(model);
    const int64_t nd = N * (int64_t)sizeof(double);
    PASSCHK(f.bind({buf_in(series, nd * T), buf_in(params, nd * K), buf_out(out, nd * (want_grad ? K : 1))}));
    RCCHK(h, f.overlap(), "overlap");
    PASSCHK(f.begin());
    RCCHK(h, sts::launch_model_eval(model, f.dev<double>(0), T, N, T, f.dev<double>(1),
                                    want_grad ? nullptr : f.dev<double>(2), want_grad ? f.dev<double>(2) : nullptr,
                                    f.s()), "model eval");
    return f.finish();
}

// what a streaming call runs: a model's pair (add 0 / 1), ARModel's pair at order p, or a sample recursion
enum { kFxPair = 0, kFxArPair = 1, kFxSample = 2 };
struct FxKind {
    int kind, model, p, add;
    int num_params() const { return kind == kFxArPair ? 1 + p : sts::model_num_params(model); }
};
int fx_check(arima_handle *h, const FxKind &k) {
    if (k.kind != kFxArPair) return ARIMA_OK;
    if (k.p < 1) return set_err(h, ARIMA_E_INVALID_ARG, "AR order below 1");
    if (k.p > sts::kGenMaxOrder) return set_err(h, ARIMA_E_UNSUPPORTED, "AR order above 20");
    return ARIMA_OK;
}
int fx_launch(const FxKind &k, const double *in, int64_t ld_in, const double *params, double *out, int64_t ld_out,
              int64_t N, int T, hipStream_t s) {
    if (k.kind == kFxArPair) return sts::launch_ar_effects(in, ld_in, params, k.p, out, ld_out, N, T, k.add, s);
    if (k.kind == kFxSample) return sts::launch_garch_sample(k.model, in, ld_in, params, out, ld_out, N, T, s);
    return sts::launch_model_effects(k.model, in, ld_in, params, out, ld_out, N, T, k.add, s);
}

int fx_body(arima_handle *h, CallFlavour flavour, const FxKind &k, const double *in, int64_t N, int32_t T, int64_t ld,
            const double *params, double *out, int64_t ld_out, void *stream) {
    if (!h) return ARIMA_E_INVALID_ARG;
    CallFrame f(h, flavour);
    if (N < 0 || T < 0 || ld < T || ld_out < T) return set_err(h, ARIMA_E_INVALID_ARG, "bad shape");
    PASSCHK(fx_check(h, k));
    if (N == 0 || T == 0) return ARIMA_OK;
    PASSCHK(f.bind({buf_in(in, strided_bytes(N, ld, T)), buf_in(params, N * k.num_params() * (int64_t)sizeof(double)),
                    buf_out(out, strided_bytes(N, ld_out, T))}));
    RCCHK(h, f.overlap(), "overlap");
    PASSCHK(f.begin(stream));
    RCCHK(h, fx_launch(k, f.dev<double>(0), ld, f.dev<double>(1), f.dev<double>(2), ld_out, N, T, f.s()),
          "model effects");
    return f.finish();
}
}  // namespace

int arima_ewma_fit_batch(arima_handle *h, const double *series, int64_t N, int32_t T, double *smoothing_out,
                         double *sse_out, int32_t *status_out, int32_t *n_eval_out, int32_t *n_grad_out) {
    return md_fit_body(h, kHostBuffers, sts::kModelEwma, series, N, T, T, smoothing_out, sse_out, status_out, n_eval_out,
                       n_grad_out, nullptr);
}

int arima_ewma_fit_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                double *d_smoothing_out, double *d_sse_out, int32_t *d_status_out,
                                int32_t *d_n_eval_out, int32_t *d_n_grad_out, void *stream) {
    return md_fit_body(h, kDeviceBuffers, sts::kModelEwma, d_series, N, T, ld, d_smoothing_out, d_sse_out, d_status_out,
                         d_n_eval_out, d_n_grad_out, stream);
}

int arima_garch_fit_batch(arima_handle *h, const double *series, int64_t N, int32_t T, double *coef_out,
                          double *ll_out, int32_t *status_out, int32_t *n_eval_out, int32_t *n_grad_out) {
    return md_fit_body(h, kHostBuffers, sts::kModelGarch, series, N, T, T, coef_out, ll_out, status_out, n_eval_out,
                       n_grad_out, nullptr);
}

int arima_garch_fit_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                 double *d_coef_out, double *d_ll_out, int32_t *d_status_out, int32_t *d_n_eval_out,
                                 int32_t *d_n_grad_out, void *stream) {
    return md_fit_body(h, kDeviceBuffers, sts::kModelGarch, d_series, N, T, ld, d_coef_out, d_ll_out, d_status_out, d_n_eval_out,
                         d_n_grad_out, stream);
}

int arima_ewma_sse_batch(arima_handle *h, const double *series, int64_t N, int32_t T, const double *smoothing,
                         double *sse_out) {
    return md_eval_host(h, sts::kModelEwma, series, N, T, smoothing, sse_out, 0);
}

int arima_ewma_gradient_batch(arima_handle *h, const double *series, int64_t N, int32_t T, const double *smoothing,
                              double *grad_out) {
    return md_eval_host(h, sts::kModelEwma, series, N, T, smoothing, grad_out, 1);
}

int arima_garch_loglik_batch(arima_handle *h, const double *series, int64_t N, int32_t T, const double *coef,
                             double *ll_out) {
    return md_eval_host(h, sts::kModelGarch, series, N, T, coef, ll_out, 0);
}

int arima_garch_gradient_batch(arima_handle *h, const double *series, int64_t N, int32_t T, const double *coef,
                               double *grad_out) {
    return md_eval_host(h, sts::kModelGarch, series, N, T, coef, grad_out, 1);
}

int arima_ewma_remove_effects_batch(arima_handle *h, const double *series, int64_t N, int32_t T,
                                    const double *smoothing, double *out) {
    return fx_body(h, kHostBuffers, FxKind{kFxPair, sts::kModelEwma, 0, 0}, series, N, T, T, smoothing, out, T, nullptr);
}

int arima_ewma_add_effects_batch(arima_handle *h, const double *series, int64_t N, int32_t T, const double *smoothing,
                                 double *out) {
    return fx_body(h, kHostBuffers, FxKind{kFxPair, sts::kModelEwma, 0, 1}, series, N, T, T, smoothing, out, T, nullptr);
}

int arima_garch_remove_effects_batch(arima_handle *h, const double *series, int64_t N, int32_t T, const double *coef,
                                     double *out) {
    return fx_body(h, kHostBuffers, FxKind{kFxPair, sts::kModelGarch, 0, 0}, series, N, T, T, coef, out, T, nullptr);
}

int arima_garch_add_effects_batch(arima_handle *h, const double *series, int64_t N, int32_t T, const double *coef,
                                  double *out) {
    return fx_body(h, kHostBuffers, FxKind{kFxPair, sts::kModelGarch, 0, 1}, series, N, T, T, coef, out, T, nullptr);
}

int arima_ewma_remove_effects_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                           const double *d_smoothing, double *d_out, int64_t ld_out, void *stream) {
    return fx_body(h, kDeviceBuffers, FxKind{kFxPair, sts::kModelEwma, 0, 0}, d_series, N, T, ld, d_smoothing, d_out, ld_out,
                   stream);
}

int arima_ewma_add_effects_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                        const double *d_smoothing, double *d_out, int64_t ld_out, void *stream) {
    return fx_body(h, kDeviceBuffers, FxKind{kFxPair, sts::kModelEwma, 0, 1}, d_series, N, T, ld, d_smoothing, d_out, ld_out,
                   stream);
}

int arima_garch_remove_effects_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                            const double *d_coef, double *d_out, int64_t ld_out, void *stream) {
    return fx_body(h, kDeviceBuffers, FxKind{kFxPair, sts::kModelGarch, 0, 0}, d_series, N, T, ld, d_coef, d_out, ld_out,
                   stream);
}

int arima_garch_add_effects_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                         const double *d_coef, double *d_out, int64_t ld_out, void *stream) {
    return fx_body(h, kDeviceBuffers, FxKind{kFxPair, sts::kModelGarch, 0, 1}, d_series, N, T, ld, d_coef, d_out, ld_out,
                   stream);
}

int arima_argarch_fit_batch(arima_handle *h, const double *series, int64_t N, int32_t T, double *coef_out,
                            double *ll_out, int32_t *status_out, int32_t *n_eval_out, int32_t *n_grad_out) {
    return md_fit_body(h, kHostBuffers, sts::kModelArGarch, series, N, T, T, coef_out, ll_out, status_out, n_eval_out,
                       n_grad_out, nullptr);
}

int arima_argarch_fit_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                   double *d_coef_out, double *d_ll_out, int32_t *d_status_out, int32_t *d_n_eval_out,
                                   int32_t *d_n_grad_out, void *stream) {
    return md_fit_body(h, kDeviceBuffers, sts::kModelArGarch, d_series, N, T, ld, d_coef_out, d_ll_out, d_status_out, d_n_eval_out,
                         d_n_grad_out, stream);
}

int arima_argarch_remove_effects_batch(arima_handle *h, const double *series, int64_t N, int32_t T, const double *coef,
                                       double *out) {
    return fx_body(h, kHostBuffers, FxKind{kFxPair, sts::kModelArGarch, 0, 0}, series, N, T, T, coef, out, T, nullptr);
}

int arima_argarch_add_effects_batch(arima_handle *h, const double *series, int64_t N, int32_t T, const double *coef,
                                    double *out) {
    return fx_body(h, kHostBuffers, FxKind{kFxPair, sts::kModelArGarch, 0, 1}, series, N, T, T, coef, out, T, nullptr);
}

int arima_argarch_remove_effects_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                              const double *d_coef, double *d_out, int64_t ld_out, void *stream) {
    return fx_body(h, kDeviceBuffers, FxKind{kFxPair, sts::kModelArGarch, 0, 0}, d_series, N, T, ld, d_coef, d_out, ld_out,
                   stream);
}

int arima_argarch_add_effects_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                           const double *d_coef, double *d_out, int64_t ld_out, void *stream) {
    return fx_body(h, kDeviceBuffers, FxKind{kFxPair, sts::kModelArGarch, 0, 1}, d_series, N, T, ld, d_coef, d_out, ld_out,
                   stream);
}

int arima_ar_remove_effects_batch(arima_handle *h, const double *series, int64_t N, int32_t T, int32_t p,
                                  const double *coef, double *out) {
    return fx_body(h, kHostBuffers, FxKind{kFxArPair, 0, p, 0}, series, N, T, T, coef, out, T, nullptr);
}

int arima_ar_add_effects_batch(arima_handle *h, const double *series, int64_t N, int32_t T, int32_t p,
                               const double *coef, double *out) {
    return fx_body(h, kHostBuffers, FxKind{kFxArPair, 0, p, 1}, series, N, T, T, coef, out, T, nullptr);
}

int arima_ar_remove_effects_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                         int32_t p, const double *d_coef, double *d_out, int64_t ld_out, void *stream) {
    return fx_body(h, kDeviceBuffers, FxKind{kFxArPair, 0, p, 0}, d_series, N, T, ld, d_coef, d_out, ld_out, stream);
}

int arima_ar_add_effects_batch_device(arima_handle *h, const double *d_series, int64_t N, int32_t T, int64_t ld,
                                      int32_t p, const double *d_coef, double *d_out, int64_t ld_out, void *stream) {
    return fx_body(h, kDeviceBuffers, FxKind{kFxArPair, 0, p, 1}, d_series, N, T, ld, d_coef, d_out, ld_out, stream);
}

int arima_garch_sample_batch(arima_handle *h, const double *z, int64_t N, int32_t T, const double *coef, double *out) {
    return fx_body(h, kHostBuffers, FxKind{kFxSample, sts::kModelGarch, 0, 0}, z, N, T, T, coef, out, T, nullptr);
}

int arima_argarch_sample_batch(arima_handle *h, const double *z, int64_t N, int32_t T, const double *coef, double *out) {
    return fx_body(h, kHostBuffers, FxKind{kFxSample, sts::kModelArGarch, 0, 0}, z, N, T, T, coef, out, T, nullptr);
}

int arima_garch_sample_batch_device(arima_handle *h, const double *d_z, int64_t N, int32_t T, int64_t ld,
                                    const double *d_coef, double *d_out, int64_t ld_out, void *stream) {
    return fx_body(h, kDeviceBuffers, FxKind{kFxSample, sts::kModelGarch, 0, 0}, d_z, N, T, ld, d_coef, d_out, ld_out, stream);
}

int arima_argarch_sample_batch_device(arima_handle *h, const double *d_z, int64_t N, int32_t T, int64_t ld,
                                      const double *d_coef, double *d_out, int64_t ld_out, void *stream) {
    return fx_body(h, kDeviceBuffers, FxKind{kFxSample, sts::kModelArGarch, 0, 0}, d_z, N, T, ld, d_coef, d_out, ld_out,
                             stream);
}

int arima_get_last_model_fit_stats(arima_handle *h, arima_model_fit_stats *out) {
    if (!h || !out) return ARIMA_E_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    memset(out, 0, sizeof *out);
    if (h->md_last_n < 0) return set_err(h, ARIMA_E_INVALID_ARG, "no EWMA / GARCH / ARGARCH fit on this handle yet");
    HIPCHK(h, hipSetDevice(h->device));
    if (h->has_done) HIPCHK(h, hipEventSynchronize(h->ev_done));
    unsigned long long w[sts::kModelCtlWords];
    HIPCHK(h, hipMemcpy(w, h->md_ctl.ptr, sizeof w, hipMemcpyDeviceToHost));
    out->n_series = h->md_last_n;
    out->wave_passes = (int64_t)w[0];
    out->lane_passes = (int64_t)w[1];
    out->max_wave_passes = (int64_t)w[2];
    return ARIMA_OK;
}

}  // extern "C"
