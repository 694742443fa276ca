// Sweeps the host-side planners of spark-timeseries_amd/csrc/host_plan.hpp (what arima_runtime.cpp sizes its device and
// pinned buffers with) on the CPU: the host path's chunk schedule against the properties every plan must have and
// against the schedule it replaced, the pinned-staging layout, the staging-arena layout, the byte-span overlap rule
// against a per-byte test and against the two tests it replaced, par_memcpy and its partition, and the slice formulas.
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

static void check_arena(const size_t *bytes, int n) {
    size_t off[8] = {}, end = 0;
    const size_t total = P::arena_layout(bytes, n, off);
    for (int i = 0; i < n; ++i) {
        if (off[i] % 256) FAIL("arena_layout: offset %d = %zu of %d regions not 256-byte aligned", i, off[i], n);
        if (off[i] < end) FAIL("arena_layout: region %d at %zu starts before the end %zu of the regions declared before it", i, off[i], end);
        if (bytes[i] == 0 && off[i] != (end + 255) / 256 * 256) FAIL("arena_layout: empty region %d at %zu takes space", i, off[i]);
        end = off[i] + bytes[i];
    }
    if (total != (end + 255) / 256 * 256) FAIL("arena_layout: size %zu of %d regions, last one ends at %zu", total, n, end);
    // without its empty regions the layout is the same
    size_t dense[8], doff[8];
    int m = 0;
    for (int i = 0; i < n; ++i)
        if (bytes[i]) dense[m++] = bytes[i];
    if (P::arena_layout(dense, m, doff) != total) FAIL("arena_layout: empty regions change the size of %d regions", n);
    for (int i = 0, j = 0; i < n; ++i)
        if (bytes[i] && doff[j++] != off[i]) FAIL("arena_layout: empty regions move region %d of %d", i, n);
}

static void sweep_arena_layout() {
    const size_t pick[8] = {0, 1, 7, 8, 255, 256, 257, 4096 + 8};
    size_t bytes[8];
    int64_t cases = 0;
    for (int n = 0; n <= 8; ++n) {               // every tuple of every count: 8^0 + ... + 8^8
        int64_t tuples = 1;
        for (int i = 0; i < n; ++i) tuples *= 8;
        for (int64_t t = 0; t < tuples; ++t, ++cases) {
            int64_t v = t;
            for (int i = 0; i < n; ++i, v /= 8) bytes[i] = pick[v % 8];
            check_arena(bytes, n);
        }
    }
    std::printf("arena_layout: all %" PRId64 " tuples of 0..8 regions aligned, disjoint, in order, empty regions free\n", cases);
}

// The two overlap tests ByteSpan::meets replaced in arima_runtime.cpp, kept here as the reference: the fit pipeline's
// [lo, hi) pairs (with the function that filled them) and the entry points' (pointer, bytes) form.
static void old_set_span(uintptr_t (&sp)[2], const void *p, int64_t bytes) {
    sp[0] = (uintptr_t)p;
    sp[1] = p && bytes > 0 ? (uintptr_t)p + (uintptr_t)bytes : (uintptr_t)p;
}
static bool old_spans_meet(const uintptr_t (&a)[2], const uintptr_t (&b)[2]) {
    return a[0] < a[1] && b[0] < b[1] && a[0] < b[1] && b[0] < a[1];
}
static bool old_spans_meet(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a_bytes > 0 && b_bytes > 0 && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

static bool bytes_shared(int s1, int l1, int s2, int l2) {
    for (int x = s1; x < s1 + l1; ++x)
        if (x >= s2 && x < s2 + l2) return true;
    return false;
}

static void sweep_spans() {
    static unsigned char arr[64 + 16];           // starts 0..63 of the first 64 bytes, lengths 0..16
    int64_t pairs = 0;
    for (int s1 = 0; s1 < 64; ++s1)
        for (int l1 = 0; l1 <= 16; ++l1)
            for (int s2 = 0; s2 < 64; ++s2)
                for (int l2 = 0; l2 <= 16; ++l2, ++pairs) {
                    const P::ByteSpan a(arr + s1, l1), b(arr + s2, l2);
                    const bool want = bytes_shared(s1, l1, s2, l2);
                    if (a.meets(b) != want || b.meets(a) != want) FAIL("meets: [%d, +%d) and [%d, +%d): expected %d", s1, l1, s2, l2, (int)want);
                    uintptr_t oa[2], ob[2];
                    old_set_span(oa, arr + s1, l1);
                    old_set_span(ob, arr + s2, l2);
                    if (old_spans_meet(oa, ob) != want || old_spans_meet(arr + s1, (size_t)l1, arr + s2, (size_t)l2) != want)
                        FAIL("the replaced overlap tests disagree at [%d, +%d) and [%d, +%d)", s1, l1, s2, l2);
                }
    // null and empty spans meet nothing, each other and themselves included
    for (int s = 0; s < 64; ++s)
        for (int l = 0; l <= 16; ++l) {
            const P::ByteSpan x(arr + s, l), null_sized(nullptr, 16), null_empty(nullptr, 0), negative(arr + s, -8), empty(arr + s, 0);
            for (const P::ByteSpan &e : {null_sized, null_empty, negative, empty})
                if (!e.empty() || e.meets(x) || x.meets(e) || e.meets(e)) FAIL("an empty span meets [%d, +%d)", s, l);
        }
    // the in/out rule on seeded draws of up to 2 inputs and 6 outputs (the most an entry point or a fit call has)
    std::mt19937_64 rng(20261021);
    int64_t refused = 0, draws = 300000;
    for (int64_t t = 0; t < draws; ++t) {
        struct R { int s, l; bool null; } in[2], out[6];
        P::ByteSpan is[2], os[6];
        const int n_in = (int)(rng() % 3), n_out = (int)(rng() % 7);
        auto draw = [&](R &r, P::ByteSpan &sp) {
            r = {(int)(rng() % 64), (int)(rng() % 17), rng() % 8 == 0};
            if (rng() % 4 == 0) r.l = (int)(rng() % 3);              // more short and empty ranges
            sp = P::ByteSpan(r.null ? nullptr : arr + r.s, r.l);
            if (r.null) r.l = 0;
        };
        for (int i = 0; i < n_in; ++i) draw(in[i], is[i]);
        for (int i = 0; i < n_out; ++i) draw(out[i], os[i]);
        bool out_in = false, out_out = false;
        for (int a = 0; a < n_out; ++a) {
            for (int b = 0; b < n_in; ++b) out_in |= bytes_shared(out[a].s, out[a].l, in[b].s, in[b].l);
            for (int b = a + 1; b < n_out; ++b) out_out |= bytes_shared(out[a].s, out[a].l, out[b].s, out[b].l);
        }
        const P::Overlap got = P::find_overlap(is, n_in, os, n_out);
        if ((got != P::kDisjoint) != (out_in || out_out)) FAIL("find_overlap: draw %" PRId64 " refused %d, bytes shared %d", t, (int)got, (int)(out_in || out_out));
        if ((got == P::kOutputMeetsInput && !out_in) || (got == P::kOutputsMeet && !out_out))
            FAIL("find_overlap: draw %" PRId64 " names violation %d, which the bytes do not show", t, (int)got);
        refused += got != P::kDisjoint;
    }
    if (refused == 0 || refused == draws) FAIL("find_overlap: the draws are all alike (%" PRId64 " refused)", refused);
    std::printf("byte spans: %" PRId64 " pairs equal the per-byte test and both replaced tests; in/out rule on %" PRId64
                " draws (%" PRId64 " refused)\n", pairs, draws, refused);
}

// strided_bytes against the elements themselves: one past the last byte of any element of N rows of `cols` elements
// that start `ld` elements apart
static void sweep_strided() {
    int64_t cases = 0;
    for (int64_t N : {0, 1, 2, 65})
        for (int64_t cols : {0, 1, 12})
            for (int64_t ld : {cols, cols + 1, cols + 4})
                for (int64_t size : {1, 4, 8}) {
                    int64_t end = 0;
                    for (int64_t i = 0; i < N; ++i)
                        for (int64_t j = 0; j < cols; ++j) end = std::max(end, (i * ld + j + 1) * size);
                    const int64_t got = P::strided_bytes(N, ld, cols, size);
                    if (got != end) FAIL("strided_bytes(%" PRId64 ", %" PRId64 ", %" PRId64 ", %" PRId64 ") = %" PRId64 ", the elements end at %" PRId64, N, ld, cols, size, got, end);
                    if (ld == cols && got != N * cols * size) FAIL("strided_bytes: dense rows span %" PRId64 ", not N * cols * size", got);
                    if (size == 8 && P::strided_bytes(N, ld, cols) != got) FAIL("strided_bytes: the default element is not a double");
                    ++cases;
                }
    std::printf("strided_bytes: %" PRId64 " shapes equal the per-element enumeration\n", cases);
}

// A buffer table against find_overlap on lists built by hand: the same verdict and the same kind
static void check_table(const char *what, const P::Buf *t, int n, const P::ByteSpan *in, int n_in, const P::ByteSpan *out,
                        int n_out, P::Overlap want) {
    const P::Overlap by_hand = P::find_overlap(in, n_in, out, n_out), got = P::table_overlap(t, n);
    if (by_hand != want) FAIL("table %s: the hand-built lists give %d, the case expects %d", what, (int)by_hand, (int)want);
    if (got != want) FAIL("table %s: table_overlap gives %d, expected %d", what, (int)got, (int)want);
    P::ByteSpan si[P::kMaxBufs], so[P::kMaxBufs];
    int ni = -1, no = -1;
    P::split_spans(t, n, si, &ni, so, &no);
    if (ni != n_in || no != n_out) FAIL("table %s: split into %d inputs and %d outputs, expected %d and %d", what, ni, no, n_in, n_out);
    for (int i = 0; i < n_in; ++i)
        if (si[i].lo != in[i].lo || si[i].hi != in[i].hi) FAIL("table %s: input %d differs from the hand-built span", what, i);
    for (int i = 0; i < n_out; ++i)
        if (so[i].lo != out[i].lo || so[i].hi != out[i].hi) FAIL("table %s: output %d differs from the hand-built span", what, i);
}

static void sweep_tables() {
    static unsigned char a[256];
    using P::ByteSpan;
    {   // a null optional output meets nothing, whatever its size
        const P::Buf t[] = {P::buf_in(a, 64), P::buf_out(a + 64, 32), P::buf_opt_out(nullptr, 64), P::buf_out(a + 96, 16)};
        const ByteSpan in[] = {ByteSpan(a, 64)}, out[] = {ByteSpan(a + 64, 32), ByteSpan(nullptr, 64), ByteSpan(a + 96, 16)};
        check_table("null optional output", t, 4, in, 1, out, 3, P::kDisjoint);
        if (P::missing_buffer(t, 4)) FAIL("a null optional output counts as missing");
    }
    {   // ... and a wanted one is an output like any other
        const P::Buf t[] = {P::buf_in(a, 64), P::buf_out(a + 64, 32), P::buf_opt_out(a + 80, 16)};
        const ByteSpan in[] = {ByteSpan(a, 64)}, out[] = {ByteSpan(a + 64, 32), ByteSpan(a + 80, 16)};
        check_table("optional output on an output", t, 3, in, 1, out, 2, P::kOutputsMeet);
    }
    {   // a zero-byte input inside an output is no overlap; the input behind it is one
        const P::Buf t[] = {P::buf_in(a + 70, 0, false), P::buf_out(a + 64, 32), P::buf_in(a + 90, 8)};
        const ByteSpan in[] = {ByteSpan(a + 70, 0), ByteSpan(a + 90, 8)}, out[] = {ByteSpan(a + 64, 32)};
        check_table("zero-byte input", t, 2, in, 1, out, 1, P::kDisjoint);
        check_table("zero-byte input, then a real one", t, 3, in, 2, out, 1, P::kOutputMeetsInput);
    }
    {   // an in-out row is written: it may meet neither an input nor another output
        const P::Buf alone[] = {P::buf_in(a, 64), P::buf_inout(a + 64, 64), P::buf_out(a + 128, 8)};
        const ByteSpan in[] = {ByteSpan(a, 64)}, out[] = {ByteSpan(a + 64, 64), ByteSpan(a + 128, 8)};
        check_table("in-out", alone, 3, in, 1, out, 2, P::kDisjoint);
        const P::Buf on_in[] = {P::buf_in(a, 64), P::buf_inout(a + 56, 64), P::buf_out(a + 128, 8)};
        const ByteSpan out2[] = {ByteSpan(a + 56, 64), ByteSpan(a + 128, 8)};
        check_table("in-out on an input", on_in, 3, in, 1, out2, 2, P::kOutputMeetsInput);
        const P::Buf on_out[] = {P::buf_in(a, 64), P::buf_inout(a + 64, 64), P::buf_out(a + 120, 8)};
        const ByteSpan out3[] = {ByteSpan(a + 64, 64), ByteSpan(a + 120, 8)};
        check_table("in-out on an output", on_out, 3, in, 1, out3, 2, P::kOutputsMeet);
    }
    {   // a needed buffer that is null is missing, an unneeded one is not
        const P::Buf t[] = {P::buf_in(nullptr, 8, false), P::buf_out(a, 8)}, u[] = {P::buf_in(a, 8), P::buf_out(nullptr, 8)};
        if (P::missing_buffer(t, 2) || !P::missing_buffer(u, 2)) FAIL("missing_buffer: needed and unneeded null buffers");
    }
    std::printf("buffer tables: split and overlap equal find_overlap on hand-built lists (null optional output, zero-byte input, in-out)\n");
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
    sweep_arena_layout();
    sweep_spans();
    sweep_strided();
    sweep_tables();
    sweep_memcpy();
    sweep_slices();
    std::printf("hostplan OK\n");
    return 0;
}
