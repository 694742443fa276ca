// Compares spark-timeseries_amd/csrc/fit_stats.hpp (the stats of the last fit as pure functions) on the CPU with the
// three bodies it replaced in arima_runtime.cpp, kept here literally as the oracle: compute_stats (a fit's stats from
// its counters), acc_stats (the sum over slices or chunks) and the order search's pair (k_search_acc per fit, then the
// search branch of arima_get_last_stats over the lanes' sums). Every field is compared bit for bit, flops included.
// Exits non-zero at the first difference. Built plain and under AddressSanitizer + UBSan (fitstats.mk).
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../spark-timeseries_amd/csrc/fit_stats.hpp"

namespace S = sts::stats;
typedef unsigned long long u64;

#define FAIL(...)                          \
    do {                                   \
        std::printf("FAIL: " __VA_ARGS__); \
        std::printf("\n");                 \
        std::exit(1);                      \
    } while (0)

constexpr int kCtlWords = 48;

// ---- the oracle: the parent's bodies (hipEventElapsedTime replaced by the four floats it returned) ----
struct PendingStats {
    bool valid = false;
    int64_t N = 0;
    int n = 0, p = 0, q = 0, I = 0;
    bool ar_only = false, user_init = false, cg = false;
    int64_t grid = 0, express = 0;
};

static arima_fit_stats old_compute_stats(const PendingStats &ps, const u64 *cc, const float *ev_ms) {
    arima_fit_stats st{};
    if (!ps.valid) return st;
    const int64_t N = ps.N;
    const int n = ps.n, p = ps.p, q = ps.q, I = ps.I, k = I + p + q;
    float ms = 0;
    ms = ev_ms[0];
    st.ms_difference = ms;
    ms = ev_ms[1];
    st.ms_hr_init = ms;
    ms = ev_ms[2];
    st.ms_cg_fit = ms;
    ms = ev_ms[3];
    st.ms_total = ms;
    st.f_passes = (int64_t)cc[1];
    st.g_passes = (int64_t)cc[2];
    st.n_eval = (int64_t)cc[5];
    st.n_grad = (int64_t)cc[6];
    st.wave_f_passes = (int64_t)cc[3];
    st.wave_g_passes = (int64_t)cc[4];
    st.spec_hits = (int64_t)cc[7];
    st.wave_multi_passes = (int64_t)cc[8];
    st.spec_chains = (int64_t)cc[9];
    st.ride_passes = (int64_t)cc[18];
    st.series_done = ps.cg ? (int64_t)cc[32] : N;
    st.express_series = (int64_t)cc[23];
    st.express_f_passes = (int64_t)cc[24];
    st.express_g_passes = (int64_t)cc[25];
    st.express_pit_passes = (int64_t)cc[33];
    st.express_pit_sweeps = (int64_t)cc[34];
    st.express_pit_g_passes = (int64_t)cc[35];
    st.wave_chains = (int64_t)cc[36];
    st.low_util_passes = (int64_t)cc[37];
    st.diag_step_cycles = (int64_t)cc[38];
    st.diag_refill_cycles = (int64_t)cc[39];
    st.merge_series = (int64_t)cc[41];
    st.merge_waves = (int64_t)cc[42];
    st.express_blocks = ps.express;
    st.fault = (int64_t)cc[26];
    for (int i = 0; i < 5; ++i) st.fault_info[i] = (int64_t)cc[27 + i];
    st.diag[0] = (int64_t)cc[10];
    st.diag[1] = (int64_t)cc[11];
    st.diag[2] = (int64_t)cc[12];
    st.diag[3] = (int64_t)cc[13];
    st.diag[4] = cc[14] ? (int64_t)(cc[14] - cc[15]) : 0;
    st.diag[5] = (int64_t)cc[16];
    st.grid_blocks = ps.grid;
    const int M = std::max(p, q), m = M + 1;
    if (ps.ar_only) st.hr_passes = N * (int64_t)(2 * (I + p) - I);
    else if (!ps.user_init) st.hr_passes = N * (int64_t)(2 * (1 + m) - 1 + 2 * k - I);
    const double S = std::max(n - M, 0);
    const double ff = 2.0 * (p + q) + 4, fg = ff + 2.0 * k * q + 1 + p + q + 2.0 * k;
    const double whr = (double)N * (3.0 * std::max(n - m, 0) * (m + 1) * (m + 1) +
                                    3.0 * std::max(n - 2 * M - 1, 0) * k * k + 2.0 * std::max(n - m, 0) * m);
    const double U = (double)(st.f_passes + st.ride_passes + st.express_f_passes + st.spec_hits);
    const double G = (double)(st.g_passes - st.ride_passes + st.express_g_passes);
    st.flops = U * S * ff + G * S * fg + (ps.user_init ? 0.0 : whr);
    st.n_series = N;
    return st;
}

static void old_acc_stats(arima_fit_stats &a, const arima_fit_stats &s) {
    a.ms_difference += s.ms_difference;
    a.ms_hr_init += s.ms_hr_init;
    a.ms_cg_fit += s.ms_cg_fit;
    a.ms_total += s.ms_total;
    a.f_passes += s.f_passes;
    a.g_passes += s.g_passes;
    a.hr_passes += s.hr_passes;
    a.n_eval += s.n_eval;
    a.n_grad += s.n_grad;
    a.flops += s.flops;
    a.n_series += s.n_series;
    a.wave_f_passes += s.wave_f_passes;
    a.wave_g_passes += s.wave_g_passes;
    a.wave_multi_passes += s.wave_multi_passes;
    a.spec_hits += s.spec_hits;
    a.spec_chains += s.spec_chains;
    a.ride_passes += s.ride_passes;
    a.series_done += s.series_done;
    a.express_series += s.express_series;
    a.express_f_passes += s.express_f_passes;
    a.express_g_passes += s.express_g_passes;
    a.express_pit_passes += s.express_pit_passes;
    a.express_pit_sweeps += s.express_pit_sweeps;
    a.express_pit_g_passes += s.express_pit_g_passes;
    a.wave_chains += s.wave_chains;
    a.low_util_passes += s.low_util_passes;
    a.merge_series += s.merge_series;
    a.merge_waves += s.merge_waves;
    a.grid_blocks = s.grid_blocks;
    a.express_blocks = s.express_blocks;
    if (!a.fault && s.fault) {
        a.fault = s.fault;
        for (int i = 0; i < 5; ++i) a.fault_info[i] = s.fault_info[i];
    }
}

static void old_k_search_acc(const u64 *ctl, u64 *acc, int64_t N, int n, int p, int q, int I, int cg) {
    for (int i = 0; i < kCtlWords; ++i)
        if (i < 26 || i > 31) acc[i] += ctl[i];
    if (acc[26] == 0 && ctl[26] != 0)
        for (int i = 26; i <= 31; ++i) acc[i] = ctl[i];
    if (!cg) acc[32] += (u64)N;
    const int k = I + p + q, M = p > q ? p : q, m = M + 1;
    const double S = n - M > 0 ? n - M : 0;
    const double ff = 2.0 * (p + q) + 4, fg = ff + 2.0 * k * q + 1 + p + q + 2.0 * k;
    const double U = (double)(ctl[1] + ctl[18] + ctl[24] + ctl[7]), G = (double)(ctl[2] - ctl[18] + ctl[25]);
    const bool ar_only = p > 0 && q == 0;
    const double whr = ar_only ? 0.0
                               : (double)N * (3.0 * (n - m > 0 ? n - m : 0) * (m + 1) * (m + 1) +
                                              3.0 * (n - 2 * M - 1 > 0 ? n - 2 * M - 1 : 0) * k * k +
                                              2.0 * (n - m > 0 ? n - m : 0) * m);
    double fl;
    memcpy(&fl, acc + kCtlWords, sizeof fl);
    fl = fl + U * S * ff + G * S * fg + whr;
    memcpy(acc + kCtlWords, &fl, sizeof fl);
}

static arima_fit_stats old_search_branch(const u64 *search_acc_host, int search_lanes_used, int64_t search_n,
                                         int64_t search_fits, int64_t last_grid, int64_t last_express, float ms) {
    arima_fit_stats st{};
    double flops = 0.0;
    u64 w[kCtlWords] = {};
    for (int j = 0; j < search_lanes_used; ++j) {
        const u64 *a = search_acc_host + (size_t)j * (kCtlWords + 1);
        for (int i = 0; i < kCtlWords; ++i)
            if (i < 26 || i > 31) w[i] += a[i];
        if (w[26] == 0 && a[26] != 0)
            for (int i = 26; i <= 31; ++i) w[i] = a[i];
        double f;
        memcpy(&f, a + kCtlWords, sizeof f);
        flops += f;
    }
    st.n_series = search_n * search_fits;
    st.f_passes = (int64_t)w[1];
    st.g_passes = (int64_t)w[2];
    st.wave_f_passes = (int64_t)w[3];
    st.wave_g_passes = (int64_t)w[4];
    st.n_eval = (int64_t)w[5];
    st.n_grad = (int64_t)w[6];
    st.spec_hits = (int64_t)w[7];
    st.wave_multi_passes = (int64_t)w[8];
    st.spec_chains = (int64_t)w[9];
    st.ride_passes = (int64_t)w[18];
    st.express_series = (int64_t)w[23];
    st.express_f_passes = (int64_t)w[24];
    st.express_g_passes = (int64_t)w[25];
    st.series_done = (int64_t)w[32];
    st.express_pit_passes = (int64_t)w[33];
    st.express_pit_sweeps = (int64_t)w[34];
    st.express_pit_g_passes = (int64_t)w[35];
    st.wave_chains = (int64_t)w[36];
    st.low_util_passes = (int64_t)w[37];
    st.merge_series = (int64_t)w[41];
    st.merge_waves = (int64_t)w[42];
    st.fault = (int64_t)w[26];
    for (int i = 0; i < 5; ++i) st.fault_info[i] = (int64_t)w[27 + i];
    st.grid_blocks = last_grid;
    st.express_blocks = last_express;
    st.flops = flops;
    st.ms_cg_fit = ms;
    st.ms_total = ms;
    return st;
}

// ---- the comparison ----
// arima_fit_stats is int64_t and double members only: 8-byte words without padding, so a word-wise comparison is the
// field-by-field one, and bit for bit for the doubles
static_assert(sizeof(arima_fit_stats) % 8 == 0, "arima_fit_stats is 8-byte words");
static void same(const arima_fit_stats &want, const arima_fit_stats &got, const char *what, long long id) {
    u64 a[sizeof(arima_fit_stats) / 8], b[sizeof(arima_fit_stats) / 8];
    memcpy(a, &want, sizeof a);
    memcpy(b, &got, sizeof b);
    for (size_t i = 0; i < sizeof(arima_fit_stats) / 8; ++i)
        if (a[i] != b[i])
            FAIL("%s case %lld: word %zu (byte offset %zu) is %#llx, the replaced body gave %#llx (flops %.17g vs %.17g)",
                 what, id, i, i * 8, b[i], a[i], got.flops, want.flops);
}

static std::mt19937_64 rng(20240607);
// counters below 2^44 (sums of 65 stay far from the int64 range), every fourth one zero; now and then more objective
// riders than gradient passes, where the fit's signed G and the search's wrapped unsigned G part ways
static void random_counters(u64 *cc, int fault) {
    for (int i = 0; i < kCtlWords; ++i) cc[i] = (rng() & 3) ? rng() >> (20 + rng() % 40) : 0;
    if (rng() % 8 == 0) cc[18] = cc[2] + cc[25] + 1 + rng() % 1000;
    cc[26] = fault;
    if (!fault)
        for (int i = 27; i <= 31; ++i) cc[i] = 0;
}

int main() {
    const int orders[] = {0, 1, 2, 3, 4, 5, 6, 20};
    long long fits = 0, sums = 0, searches = 0;
    std::vector<PendingStats> shapes;
    for (int p : orders)
        for (int q : orders)
            for (int I = 0; I <= 1; ++I) {
                const int M = std::max(p, q);
                // n from 0 to above 2M + 1: each of max(n - M, 0), max(n - m, 0), max(n - 2M - 1, 0) clamps and not
                for (int n : {0, 1, M - 1, M, M + 1, M + 2, 2 * M, 2 * M + 1, 2 * M + 2, 2 * M + 9, 64, 1024, 4096}) {
                    if (n < 0) continue;
                    for (int f = 0; f < 9; ++f) {
                        PendingStats ps;
                        ps.valid = f < 8;
                        ps.ar_only = f & 1;
                        ps.user_init = f & 2;
                        ps.cg = f & 4;
                        ps.N = (rng() % 4 == 0) ? 0 : (int64_t)(rng() >> (31 + rng() % 30));
                        ps.n = n, ps.p = p, ps.q = q, ps.I = I;
                        ps.grid = rng() % 2048, ps.express = rng() % 64;
                        shapes.push_back(ps);
                    }
                }
            }
    auto to_shape = [](const PendingStats &ps) {
        S::FitShape sh;
        sh.valid = ps.valid, sh.N = ps.N, sh.n = ps.n, sh.p = ps.p, sh.q = ps.q, sh.I = ps.I;
        sh.ar_only = ps.ar_only, sh.user_init = ps.user_init, sh.cg = ps.cg, sh.grid = ps.grid, sh.express = ps.express;
        return sh;
    };
    auto one_fit = [&](const PendingStats &ps, int fault, arima_fit_stats *want, arima_fit_stats *got) {
        u64 cc[kCtlWords];
        random_counters(cc, fault);
        const float ms[4] = {(float)(rng() % 100000) / 977.0f, (float)(rng() % 100000) / 313.0f,
                             (float)(rng() % 100000) / 71.0f, (float)(rng() % 100000) / 13.0f};
        *want = old_compute_stats(ps, cc, ms);
        *got = S::fit_stats(to_shape(ps), cc, S::FitTimes{ms[0], ms[1], ms[2], ms[3]});
    };
    // (1) a fit's stats from its counters: every shape, with and without a fault record
    for (const PendingStats &ps : shapes)
        for (int fault : {0, 2}) {
            arima_fit_stats want, got;
            one_fit(ps, fault, &want, &got);
            same(want, got, "fit_stats", fits++);
        }
    // (2) sums of 1, 2 and 65 records with a fault record in the first, a middle or no summand (a later summand's
    // second fault must not replace the first)
    for (int count : {1, 2, 65})
        for (int where : {-1, 0, count / 2})
            for (int rep = 0; rep < 200; ++rep) {
                arima_fit_stats want{}, got{};
                for (int j = 0; j < count; ++j) {
                    const int fault = where < 0 ? 0 : (j == where ? 1 : (j > where && j % 7 == 0 ? 3 : 0));
                    arima_fit_stats w1, g1;
                    one_fit(shapes[rng() % shapes.size()], fault, &w1, &g1);
                    old_acc_stats(want, w1);
                    S::acc_stats(got, g1);
                    same(want, got, "acc_stats", sums);
                }
                ++sums;
            }
    // (3) the order search: 1, 2 and 65 fits dealt over 1, 2 and 8 lanes, each into its lane's sums, then the lanes'
    // sums into the stats; cg = 0 (no counters, every series written) and 1
    for (int count : {1, 2, 65})
        for (int lanes : {1, 2, 8})
            for (int where : {-1, 0, count / 2})
                for (int rep = 0; rep < 100; ++rep) {
                    std::vector<u64> want_acc((size_t)lanes * (kCtlWords + 1), 0), got_acc(want_acc);
                    const int64_t N = (int64_t)(rng() >> (31 + rng() % 30));
                    for (int j = 0; j < count; ++j) {
                        const PendingStats &ps = shapes[rng() % shapes.size()];
                        const int fault = where < 0 ? 0 : (j == where ? 2 : (j > where && j % 5 == 0 ? 1 : 0));
                        u64 cc[kCtlWords];
                        random_counters(cc, fault);
                        const int cg = ps.cg ? 1 : 0;
                        if (!cg) memset(cc, 0, sizeof cc);
                        const size_t at = (size_t)(j % lanes) * (kCtlWords + 1);
                        old_k_search_acc(cc, &want_acc[at], N, ps.n, ps.p, ps.q, ps.I, cg);
                        S::search_acc_fit(cc, &got_acc[at], N, ps.n, ps.p, ps.q, ps.I, cg);
                    }
                    if (want_acc != got_acc) FAIL("search_acc_fit case %lld: the lanes' sums differ", searches);
                    const int64_t grid = rng() % 2048, express = rng() % 64;
                    const float ms = (float)(rng() % 100000) / 37.0f;
                    same(old_search_branch(want_acc.data(), lanes, N, count, grid, express, ms),
                         S::search_stats(got_acc.data(), lanes, N * count, grid, express, ms), "search_stats", searches++);
                }
    // the names are the words the kernels write
    static_assert(S::kCtlWords == kCtlWords && S::kCtlFault == 26 && S::kCtlFaultLast == 31 && S::kCtlSeriesDone == 32,
                  "counter words");
    std::printf("fits %lld sums %lld searches %lld\nfitstats OK\n", fits, sums, searches);
    return 0;
}
