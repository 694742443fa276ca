// Sweeps the host-side planners of spark-timeseries_amd/csrc/host_plan.hpp (what arima_runtime.cpp sizes its device and
// pinned buffers with) on the CPU: the host path's chunk schedule against the properties every plan must have and
// against the schedule it replaced, the pinned-staging layout, par_memcpy and its partition, and the slice formulas.
// Exits non-zero at the first offending tuple. Built plain and under AddressSanitizer + UBSan (hostplan.mk).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../spark-timeseries_amd/csrc/host_plan.hpp"

namespace P = sts::plan;
using std::vector;

#define FAIL(...)                          \
    do {                                   \
        std::printf("FAIL: " __VA_ARGS__); \
        std::printf("\n");                 \
        std::exit(1);                      \
    } while (0)

// The schedule before the tail chunk was clamped to host_chunk, kept here as the reference: wherever it stays within
// min(host_chunk, N) the planner must reproduce it element for element.
static vector<int64_t> old_starts(int64_t N, int64_t host_chunk, int host_tail) {
    const int64_t chunk = std::min<int64_t>(host_chunk, N);
    vector<int64_t> starts;
    for (int64_t f = 0; f < N;) {
        starts.push_back(f);
        const int64_t rem = N - f;
        int64_t n = std::min(chunk, rem);
        if (host_tail && rem <= 2 * chunk && rem > 16384) n = std::max<int64_t>(16384, (rem + 1) / 2);
        f += n;
    }
    starts.push_back(N);
    return starts;
}

static vector<int64_t> sizes(const vector<int64_t> &st) {
    vector<int64_t> s;
    for (size_t j = 0; j + 1 < st.size(); ++j) s.push_back(st[j + 1] - st[j]);
    return s;
}

static void check_plan(int64_t N, int64_t hc, int64_t *old_overruns, int64_t *new_overruns) {
    const int64_t cap = std::min(hc, N);
    const vector<int64_t> flat = P::host_chunk_starts(N, hc, 0);
    for (int tail = 0; tail <= 1; ++tail) {
        const vector<int64_t> st = P::host_chunk_starts(N, hc, tail);
        if (st.empty() || st.back() != N) FAIL("plan N=%" PRId64 " chunk=%" PRId64 " tail=%d does not end at N", N, hc, tail);
        if (N == 0) {
            if (st.size() != 1) FAIL("plan N=0 chunk=%" PRId64 " tail=%d is not just the terminator", hc, tail);
            continue;
        }
        if (st[0] != 0) FAIL("plan N=%" PRId64 " chunk=%" PRId64 " tail=%d does not start at 0", N, hc, tail);
        const vector<int64_t> sz = sizes(st);
        bool over = false;
        for (size_t j = 0; j < sz.size(); ++j) {
            if (sz[j] < 1) FAIL("plan N=%" PRId64 " chunk=%" PRId64 " tail=%d: chunk %zu has %" PRId64 " series", N, hc, tail, j, sz[j]);
            if (sz[j] > cap) over = true;
            if (!tail && j + 1 < sz.size() && sz[j] != cap)
                FAIL("plan N=%" PRId64 " chunk=%" PRId64 " tail=0: chunk %zu is %" PRId64 ", not %" PRId64, N, hc, j, sz[j], cap);
        }
        if (over) {
            ++*new_overruns;
            FAIL("plan N=%" PRId64 " chunk=%" PRId64 " tail=%d exceeds min(host_chunk, N)", N, hc, tail);
        }
        if (P::max_chunk(st) != *std::max_element(sz.begin(), sz.end()))
            FAIL("max_chunk N=%" PRId64 " chunk=%" PRId64 " tail=%d", N, hc, tail);
        if (tail) {
            // where the two plans hold different sizes at the same index, the tail plan's is at least kHostTailMin --
            // unless it is the plan's last chunk, the remainder, which is whatever is left (13616 in
            // (70000, 20000) -> [20000, 20000, 16384, 13616])
            const vector<int64_t> fz = sizes(flat);
            for (size_t j = 0; j < sz.size(); ++j) {
                const bool differs = j >= fz.size() || fz[j] != sz[j];
                if (differs && sz[j] < P::kHostTailMin && j + 1 < sz.size())
                    FAIL("plan N=%" PRId64 " chunk=%" PRId64 " tail=1: chunk %zu (%" PRId64 ") differs from the flat plan below the floor", N,
                         hc, j, sz[j]);
            }
        }
        const vector<int64_t> old = old_starts(N, hc, tail);
        const vector<int64_t> oz = sizes(old);
        const bool old_over = *std::max_element(oz.begin(), oz.end()) > cap;
        if (old_over) {
            if (tail) ++*old_overruns;
            else FAIL("the flat reference schedule overruns at N=%" PRId64 " chunk=%" PRId64, N, hc);
        } else if (old != st) {
            FAIL("plan N=%" PRId64 " chunk=%" PRId64 " tail=%d differs from the previous schedule where that one was in bounds", N, hc,
                 tail);
        }
    }
}

static void expect_plan(int64_t N, int64_t hc, const vector<int64_t> &want) {
    const vector<int64_t> got = sizes(P::host_chunk_starts(N, hc, 1));
    if (got != want || sizes(old_starts(N, hc, 1)) != want) {
        std::printf("FAIL: literal plan N=%" PRId64 " chunk=%" PRId64 ": got [", N, hc);
        for (int64_t v : got) std::printf(" %" PRId64, v);
        std::printf(" ]\n");
        std::exit(1);
    }
}

static void sweep_chunks() {
    vector<int64_t> hcs, Ns;
    for (int64_t c = 1; c <= 40000; c += 97) hcs.push_back(c);
    for (int64_t c : {8192, 8193, 10000, 16383, 16384, 16385, 1 << 17, 1 << 18}) hcs.push_back(c);
    for (int64_t n = 1; n <= 90000; n += 389) Ns.push_back(n);
    for (int64_t n : {0, 1, 16384, 16385, 20000, 32768, 32769, 1 << 20}) Ns.push_back(n);
    int64_t old_over = 0, new_over = 0, lo = INT64_MAX, hi = 0;
    for (int64_t hc : hcs)
        for (int64_t N : Ns) {
            const int64_t before = old_over;
            check_plan(N, hc, &old_over, &new_over);
            if (old_over != before) {
                lo = std::min(lo, hc);
                hi = std::max(hi, hc);
            }
        }
    // the three tuples of the overrun report
    struct { int64_t N, hc; vector<int64_t> old, now; } known[] = {
        {20000, 10000, {16384, 3616}, {10000, 10000}},
        {16385, 9000, {16384, 1}, {9000, 7385}},
        {40000, 16383, {16383, 16384, 7233}, {16383, 16383, 7234}},
    };
    for (auto &kn : known) {
        if (sizes(old_starts(kn.N, kn.hc, 1)) != kn.old) FAIL("previous schedule at N=%" PRId64 " chunk=%" PRId64, kn.N, kn.hc);
        if (sizes(P::host_chunk_starts(kn.N, kn.hc, 1)) != kn.now) FAIL("clamped schedule at N=%" PRId64 " chunk=%" PRId64, kn.N, kn.hc);
    }
    if (sizes(P::host_chunk_starts(70000, 20000, 1)) != vector<int64_t>{20000, 20000, 16384, 13616}) FAIL("plan (70000, 20000)");
    expect_plan(1 << 20, 1 << 18, {262144, 262144, 262144, 131072, 65536, 32768, 16384, 16384});
    expect_plan(1 << 20, 1 << 17, {131072, 131072, 131072, 131072, 131072, 131072, 131072, 65536, 32768, 16384, 16384});
    if (old_over <= 0) FAIL("the previous schedule overran nowhere: the sweep misses the defect it is there to show");
    if (lo < 8193 || hi > 16383) FAIL("previous schedule overruns at host_chunk %" PRId64 "..%" PRId64 ", expected within 8193..16383", lo, hi);
    std::printf("chunk plans: %zu x %zu pairs, previous schedule overruns %" PRId64 " (host_chunk %" PRId64 "..%" PRId64
                "), new planner overruns %" PRId64 "\n", hcs.size(), Ns.size(), old_over, lo, hi, new_over);
}

static void sweep_pin_layout() {
    const int64_t ns[] = {1, 63, 64, 65, 255, 256, 257, 10000, 16384};
    for (int k = 0; k <= 11; ++k) {
        size_t prev = 0;
        for (int64_t n : ns) {
            size_t off[6];
            const size_t total = P::pin_layout(n, k, off);
            // what the host path copies into each region: n*k coefficients (k = 0: nothing), ll, three int32, flags
            const size_t pay[6] = {(size_t)n * k * 8, (size_t)n * 8, (size_t)n * 4, (size_t)n * 4, (size_t)n * 4, (size_t)n};
            for (int i = 0; i < 6; ++i) {
                if (off[i] % 256) FAIL("pin_layout(%" PRId64 ", %d): offset %d = %zu not 256-byte aligned", n, k, i, off[i]);
                if (off[i] + pay[i] > total) FAIL("pin_layout(%" PRId64 ", %d): region %d ends past the size %zu", n, k, i, total);
                for (int j = 0; j < i; ++j)
                    if (off[j] + pay[j] > off[i] && off[i] + pay[i] > off[j] && pay[i] && pay[j])
                        FAIL("pin_layout(%" PRId64 ", %d): regions %d and %d overlap", n, k, j, i);
                if (i && off[i] < off[i - 1] + pay[i - 1]) FAIL("pin_layout(%" PRId64 ", %d): region %d starts inside %d", n, k, i, i - 1);
            }
            if (total < prev) FAIL("pin_layout(%" PRId64 ", %d): size %zu below the size of a smaller n (%zu)", n, k, total, prev);
            prev = total;
        }
    }
    // monotone in n one step at a time around the 256-byte roundings too
    for (int k : {0, 1, 5, 11})
        for (int64_t n = 1; n < 2100; ++n) {
            size_t a[6], b[6];
            if (P::pin_layout(n + 1, k, b) < P::pin_layout(n, k, a)) FAIL("pin_layout not monotone at n=%" PRId64 " k=%d", n, k);
        }
    std::printf("pin_layout: aligned, disjoint, inside the size, monotone in n\n");
}

static void sweep_memcpy() {
    const size_t MiB = size_t(1) << 20;
    const size_t sizes_b[] = {0, 1, 63, 64, 65, 4 * MiB - 1, 4 * MiB, 8 * MiB, 8 * MiB + 1, 37 * MiB + 13};
    const int threads[] = {0, 1, 2, 3, 7, 16, 64};
    const size_t guard = 256;
    const size_t big = 37 * MiB + 13;
    vector<unsigned char> src(big);
    std::mt19937_64 rng(20261019);
    for (size_t i = 0; i + 8 <= big; i += 8) {
        const uint64_t v = rng();
        std::memcpy(&src[i], &v, 8);
    }
    for (size_t i = big / 8 * 8; i < big; ++i) src[i] = (unsigned char)rng();
    for (size_t bytes : sizes_b)
        for (int t : threads) {
            const auto parts = P::memcpy_parts(bytes, t);
            if ((int)parts.size() > std::max(t, 1)) FAIL("memcpy_parts(%zu, %d): %zu parts", bytes, t, parts.size());
            size_t at = 0;
            for (const auto &pt : parts) {
                if (pt.first != at || pt.second == 0) FAIL("memcpy_parts(%zu, %d): part at %zu len %zu, expected start %zu", bytes, t, pt.first, pt.second, at);
                at += pt.second;
            }
            if (at != bytes) FAIL("memcpy_parts(%zu, %d) covers %zu bytes", bytes, t, at);
            // the real copy into an exact-size heap block (so that the sanitizer build sees any byte outside it) that
            // sits between two sentinel blocks of its own
            vector<unsigned char> dst(guard + bytes + guard, 0xA5);
            unsigned char *exact = (unsigned char *)std::malloc(bytes ? bytes : 1);
            P::par_memcpy(exact, src.data(), bytes, t);
            if (bytes && std::memcmp(exact, src.data(), bytes)) FAIL("par_memcpy(%zu, %d): exact-size copy differs", bytes, t);
            std::free(exact);
            P::par_memcpy(dst.data() + guard, src.data(), bytes, t);
            if (bytes && std::memcmp(dst.data() + guard, src.data(), bytes)) FAIL("par_memcpy(%zu, %d): copy differs", bytes, t);
            for (size_t i = 0; i < guard; ++i)
                if (dst[i] != 0xA5 || dst[guard + bytes + i] != 0xA5) FAIL("par_memcpy(%zu, %d): sentinel %zu overwritten", bytes, t, i);
        }
    std::printf("memcpy_parts / par_memcpy: exact tilings, at most `threads` parts, copies identical, sentinels intact\n");
}

static void sweep_slices() {
    const int64_t bytes[] = {1, 4096, int64_t(1) << 20, int64_t(1) << 30, int64_t(1) << 40};
    const int64_t lds[] = {16, 48, 1024, 1040, 4096 + 16};
    for (int64_t b : bytes)
        for (int64_t ld : lds) {
            const int64_t row = ld * 8;
            const struct { int64_t rows, g; const char *name; } r[] = {{P::fit_slice_rows(b, ld), 1024, "fit_slice_rows"},
                                                                    {P::diag_slice_rows(b, ld), 64, "diag_slice_rows"}};
            for (const auto &x : r) {
                if (x.rows <= 0 || x.rows % x.g) FAIL("%s(%" PRId64 ", %" PRId64 ") = %" PRId64 ": no positive multiple of %" PRId64, x.name, b, ld, x.rows, x.g);
                const bool fits = x.rows * row <= b;
                const bool next_fits = (x.rows + x.g) * row <= b;
                if (fits && next_fits) FAIL("%s(%" PRId64 ", %" PRId64 ") = %" PRId64 ": a larger multiple fits", x.name, b, ld, x.rows);
                if (!fits && x.rows != x.g) FAIL("%s(%" PRId64 ", %" PRId64 ") = %" PRId64 " exceeds the bytes and is not the floor", x.name, b, ld, x.rows);
            }
        }
    std::printf("slice rows: largest multiple of the granule that fits, or the floor\n");
}

int main() {
    sweep_chunks();
    sweep_pin_layout();
    sweep_memcpy();
    sweep_slices();
    std::printf("hostplan OK\n");
    return 0;
}
