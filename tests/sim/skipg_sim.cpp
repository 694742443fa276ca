// skipg_sim.cpp — TEST INFRASTRUCTURE: the fit kernels' optimizer state machine (cg_lane.hpp) with and without the
// skipped dead gradient (CGLane's SKIPG: after a line search whose result the next top-of-iteration test is going to
// stop on -- converged, MaxIter or MaxEval -- no gradient request is posted), run on the CPU against the CPU
// restatement (oracle/arima_oracle.c), as a stand-alone program:
//   skipg_sim <rows.f64> N T p d q I
// rows.f64: N x T raw doubles (the undifferenced series). For both smear readings and speculation off (0, 0) and on
// (2, 4) every series is fitted by the restatement (orc_fit_batch) and by both machines from the Hannan-Rissanen init.
//   - both machines against the restatement, bit for bit: status, coefficients, LL, n_eval, n_grad (builds with the
//     reference's limits only);
//   - the machines against each other, bit for bit: those, and iter, prev_obj and the point of failed fits too;
//   - a fit with status OK posts n_grad - 1 gradient requests with the skip and n_grad without it, and skips once.
// Builds with lowered limits (skipg.mk: -DSTS_CG_MAX_EVAL / -DSTS_CG_MAX_ITER) make fits stop at the top of an
// iteration on MaxEval or MaxIter within milliseconds; there the restatement (whose limits are the reference's) is
// left out and the machine without the skip is the reference. Exits non-zero at the first difference.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../spark-timeseries_amd/csrc/cg_lane.hpp"

extern "C" double orc_loglik_css_arma(const double *y, int n, int p, int q, int I, const double *coef);
extern "C" void orc_gradient_css_arma(const double *y, int n, int p, int q, int I, const double *coef, int smear,
                                      double *grad);
extern "C" void orc_differences_of_order_d(const double *ts, int n, int d, double *out);
extern "C" int orc_hannan_rissanen(const double *y, int n, int p, int q, int I, double *out);
extern "C" int orc_fit_batch(const double *series, long long N, int T, int p, int d, int q, int I, int method,
                             const double *user_init, int smear, double *coef, double *ll, int *status, int *counters);

#define FAIL(...)                          \
    do {                                   \
        std::printf("FAIL: " __VA_ARGS__); \
        std::printf("\n");                 \
        std::exit(1);                      \
    } while (0)

namespace {

constexpr bool kRefLimits = sts::kMaxEval == 10000 && sts::kMaxIter == 10000;
constexpr int kMaxK = 11;

struct Fit {
    int status = 0, n_eval = 0, n_grad = 0, iter = 0, g_requests = 0, f_requests = 0, skipped = 0;
    double point[kMaxK] = {}, prev_obj = 0.0;
};

long long bits(double x) {
    long long b;
    memcpy(&b, &x, sizeof b);
    return b;
}

template <int K, int NS, int NC, bool SKIPG>
Fit run_one(const double *y, int n, int p, int q, int I, int smear, const double *init) {
    sts::CGLane<K, NS, NC, true, sts::KDim<K>, SKIPG> L;
    double x0[K];
    for (int i = 0; i < K; ++i) x0[i] = init[i];
    L.start(x0);
    double fr = 0.0, gr[K] = {};
    Fit r;
    for (;;) {
        L.advance(fr, gr);
        if (L.done()) break;
        if (L.req == sts::REQ_NONE) FAIL("the machine neither finished nor posted a request (pc %d)", (int)L.pc);
        double c[K];
        L.request_point(c);
        fr = orc_loglik_css_arma(y, n, p, q, I, c);
        if (L.req == sts::REQ_G) {
            orc_gradient_css_arma(y, n, p, q, I, c, smear, gr);
            r.g_requests++;
        } else {
            for (int h = 0; h < L.rq_nspec; ++h) {
                double cs[K];
                L.spec_point(h, cs);
                L.spec_store(h, orc_loglik_css_arma(y, n, p, q, I, cs));
            }
            r.f_requests++;
        }
        L.req = sts::REQ_NONE;
    }
    r.status = L.status;
    r.n_eval = L.n_eval;
    r.n_grad = L.n_grad;
    r.iter = L.iter;
    r.skipped = L.skipped_g;
    r.prev_obj = L.prev_obj;
    for (int i = 0; i < K; ++i) r.point[i] = L.point[i];
    return r;
}

struct Tally {
    long long fits = 0, ok = 0, top_max_eval = 0, top_max_iter = 0, skipped = 0, g_saved = 0;
};

template <int K, int NS, int NC>
void run_policy(const std::vector<double> &rows, int N, int T, int p, int d, int q, int I, int smear, Tally &t) {
    const int n = T - d;
    std::vector<double> ocoef((size_t)N * K), oll(N);
    std::vector<int> ost(N), ocnt((size_t)N * 3);
    if (kRefLimits) orc_fit_batch(rows.data(), N, T, p, d, q, I, 0, nullptr, smear, ocoef.data(), oll.data(), ost.data(), ocnt.data());
    std::vector<double> diff(T);
    for (int i = 0; i < N; ++i) {
        orc_differences_of_order_d(rows.data() + (size_t)i * T, T, d, diff.data());
        const double *y = diff.data() + d;
        double x0[K];
        if (orc_hannan_rissanen(y, n, p, q, I, x0) != 0) continue;      // no optimizer run: the init's status
        const Fit a = run_one<K, NS, NC, true>(y, n, p, q, I, smear, x0);
        const Fit b = run_one<K, NS, NC, false>(y, n, p, q, I, smear, x0);
        const char *what = nullptr;
        // the skip against the machine stepped without it: everything the kernels report or carry on
        if (a.status != b.status) what = "status";
        else if (a.n_eval != b.n_eval) what = "n_eval";
        else if (a.n_grad != b.n_grad) what = "n_grad";
        else if (a.iter != b.iter) what = "iter";
        else if (bits(a.prev_obj) != bits(b.prev_obj)) what = "prev_obj";
        for (int j = 0; j < K && !what; ++j)
            if (bits(a.point[j]) != bits(b.point[j])) what = "point";
        if (what)
            FAIL("series %d (%d,%d,%d)+%d smear %d spec (%d,%d): %s differs with the skip (status %d / %d, n_eval %d / %d, "
                 "n_grad %d / %d)", i, p, d, q, I, smear, NS, NC, what, a.status, b.status, a.n_eval, b.n_eval, a.n_grad,
                 b.n_grad);
        if (b.skipped != 0) FAIL("series %d: the machine without the skip counted one", i);
        if (a.g_requests + a.skipped != b.g_requests || a.f_requests != b.f_requests)
            FAIL("series %d: requests G %d + skipped %d / %d, F %d / %d", i, a.g_requests, a.skipped, b.g_requests,
                 a.f_requests, b.f_requests);
        if (a.skipped > 1) FAIL("series %d: %d skips in one fit", i, a.skipped);
        if (a.status == ARIMA_ST_OK) {
            // a converged fit ran at least one line search; its last gradient is the dead one
            if (a.skipped != 1 || a.g_requests != a.n_grad - 1 || b.g_requests != b.n_grad)
                FAIL("series %d: status OK with n_grad %d posted %d gradient requests (%d without the skip), skipped %d", i,
                     a.n_grad, a.g_requests, b.g_requests, a.skipped);
            t.ok++;
        } else if (a.skipped) {
            // only MaxIter and MaxEval stop a fit at the top of an iteration with a failure
            if (a.status == ARIMA_ST_MAX_EVAL) t.top_max_eval++;
            else if (a.status == ARIMA_ST_MAX_ITER) t.top_max_iter++;
            else FAIL("series %d: a skip before status %d", i, a.status);
        }
        t.skipped += a.skipped;
        t.g_saved += b.g_requests - a.g_requests;
        t.fits++;
        if (kRefLimits) {
            // against the restatement (failed fits report NaN coefficients and LL: only status and counts compare)
            const bool ok = a.status == ARIMA_ST_OK;
            if (a.status != ost[i] || a.n_eval != ocnt[(size_t)i * 3] || a.n_grad != ocnt[(size_t)i * 3 + 1])
                FAIL("series %d (%d,%d,%d)+%d smear %d spec (%d,%d): status %d n_eval %d n_grad %d, the restatement has %d "
                     "%d %d", i, p, d, q, I, smear, NS, NC, a.status, a.n_eval, a.n_grad, ost[i], ocnt[(size_t)i * 3],
                     ocnt[(size_t)i * 3 + 1]);
            if (ok) {
                for (int j = 0; j < K; ++j)
                    if (bits(a.point[j]) != bits(ocoef[(size_t)i * K + j]))
                        FAIL("series %d: coefficient %d is %.17g, the restatement has %.17g", i, j, a.point[j],
                             ocoef[(size_t)i * K + j]);
                if (bits(a.prev_obj) != bits(oll[i])) FAIL("series %d: LL %.17g, the restatement has %.17g", i, a.prev_obj, oll[i]);
            }
        }
    }
}

template <int K>
void run_order(const std::vector<double> &rows, int N, int T, int p, int d, int q, int I, Tally &t) {
    for (int smear : {1, 0}) {
        run_policy<K, 0, 0>(rows, N, T, p, d, q, I, smear, t);
        run_policy<K, 2, 4>(rows, N, T, p, d, q, I, smear, t);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 8) FAIL("usage: skipg_sim rows.f64 N T p d q I");
    const int N = std::atoi(argv[2]), T = std::atoi(argv[3]), p = std::atoi(argv[4]), d = std::atoi(argv[5]),
              q = std::atoi(argv[6]), I = std::atoi(argv[7]);
    if (N <= 0 || T <= d) FAIL("shape");
    std::vector<double> rows((size_t)N * T);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(rows.data(), sizeof(double), rows.size(), f) != rows.size()) FAIL("cannot read %s", argv[1]);
    std::fclose(f);
    Tally t;
    switch (I + p + q) {
    case 3: run_order<3>(rows, N, T, p, d, q, I, t); break;
    case 5: run_order<5>(rows, N, T, p, d, q, I, t); break;
    case 11: run_order<11>(rows, N, T, p, d, q, I, t); break;
    default: FAIL("parameter count %d is not compiled in", I + p + q);
    }
    std::printf("limits %d %d fits %lld ok %lld top_max_eval %lld top_max_iter %lld skipped %lld g_saved %lld\nskipg OK\n",
                sts::kMaxEval, sts::kMaxIter, t.fits, t.ok, t.top_max_eval, t.top_max_iter, t.skipped, t.g_saved);
    return 0;
}
