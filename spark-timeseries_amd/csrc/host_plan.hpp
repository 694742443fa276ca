// host_plan.hpp — the host-side sizing arithmetic of arima_runtime.cpp as pure functions: the host path's chunk
// schedule, the layout of one chunk's results in pinned staging, the layout of a host-buffer call's staged arrays, the
// byte-span overlap rule of the entry points, the extent of a strided buffer and the buffer table the entry points
// derive their null check, overlap check and staging from, the partition par_memcpy hands its threads, and the rows per
// slice of the sliced device fit, of the residual diagnostics and of the design-matrix regressions. No HIP headers: a CPU program
// includes this file and sweeps the functions (tests/sim/hostplan_sim.cpp). arima_runtime.cpp keeps no second copy of
// the formulas.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>

namespace sts {
namespace plan {

// smallest chunk the tail schedule (option "host_tail") cuts
constexpr int64_t kHostTailMin = 16384;

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// Chunk boundaries of the host path (arima_fit_batch): starts[0] = 0, ..., starts.back() = N; chunk j holds the series
// [starts[j], starts[j + 1]). Full chunks of min(host_chunk, N) series, then (host_tail) the last two chunks' worth
// halved again and again, down to kHostTailMin series. The call ends with the fit of its last chunk, whose duration
// is that chunk's slowest series: a small last chunk exposes less of it after the final upload. No chunk exceeds
// min(host_chunk, N): a host_chunk below kHostTailMin keeps its own size in the tail.
inline std::vector<int64_t> host_chunk_starts(int64_t N, int64_t host_chunk, int host_tail) {
    std::vector<int64_t> starts;
    const int64_t chunk = std::min<int64_t>(std::max<int64_t>(host_chunk, 1), N);
    for (int64_t f = 0; f < N;) {
        starts.push_back(f);
        const int64_t rem = N - f;
        int64_t n = std::min(chunk, rem);
        if (host_tail && rem <= 2 * chunk && rem > kHostTailMin)
            n = std::min(chunk, std::max<int64_t>(kHostTailMin, (rem + 1) / 2));
        f += n;
    }
    starts.push_back(std::max<int64_t>(N, 0));
    return starts;
}

// largest chunk of a plan (what every per-context buffer of the host path is sized for)
inline int64_t max_chunk(const std::vector<int64_t> &starts) {
    int64_t m = 0;
    for (size_t j = 0; j + 1 < starts.size(); ++j) m = std::max(m, starts[j + 1] - starts[j]);
    return m;
}

// bytes of one chunk's results in pinned staging: coef (n*k), ll, status, n_eval, n_grad, flags
inline size_t pin_layout(int64_t n, int k, size_t off[6]) {
    size_t o = 0;
    off[0] = o; o += round_up((int64_t)n * std::max(k, 1) * 8, 256);
    off[1] = o; o += round_up(n * 8, 256);
    off[2] = o; o += round_up(n * 4, 256);
    off[3] = o; o += round_up(n * 4, 256);
    off[4] = o; o += round_up(n * 4, 256);
    off[5] = o; o += round_up(n, 256);
    return o;
}

// The staged arrays of one host-buffer call in one device block (the same idea as pin_layout, for any set of arrays):
// region i of bytes[i] bytes starts at off[i], a multiple of 256, in declaration order; a zero-byte region takes no
// space. Returns the block's size.
inline size_t arena_layout(const size_t *bytes, int n, size_t *off) {
    size_t o = 0;
    for (int i = 0; i < n; ++i) {
        off[i] = o;
        o += (bytes[i] + 255) / 256 * 256;
    }
    return o;
}

// A caller's buffer as a byte range. A null pointer or a non-positive size makes it empty, and an empty span meets
// nothing.
struct ByteSpan {
    uintptr_t lo = 0, hi = 0;
    ByteSpan() = default;
    ByteSpan(const void *p, int64_t bytes)
        : lo((uintptr_t)p), hi(p && bytes > 0 ? (uintptr_t)p + (uintptr_t)bytes : (uintptr_t)p) {}
    bool empty() const { return lo >= hi; }
    bool meets(const ByteSpan &o) const { return !empty() && !o.empty() && lo < o.hi && o.lo < hi; }
};

// The rule of every entry point that checks its buffers: no output meets an input, no two outputs meet.
enum Overlap { kDisjoint = 0, kOutputMeetsInput, kOutputsMeet };
inline Overlap find_overlap(const ByteSpan *in, int n_in, const ByteSpan *out, int n_out) {
    for (int a = 0; a < n_out; ++a) {
        for (int b = 0; b < n_in; ++b)
            if (out[a].meets(in[b])) return kOutputMeetsInput;
        for (int b = a + 1; b < n_out; ++b)
            if (out[a].meets(out[b])) return kOutputsMeet;
    }
    return kDisjoint;
}

// Bytes a caller's N rows of `cols` elements span when consecutive rows start `ld` elements apart (ld >= cols): from the
// first element of row 0 to the last of row N - 1. At ld == cols that is N * cols * size. No rows, or rows of no
// elements, span nothing.
inline int64_t strided_bytes(int64_t N, int64_t ld, int64_t cols, int64_t size = 8) {
    return N <= 0 || cols <= 0 ? 0 : ((N - 1) * ld + cols) * size;
}

// One buffer argument of an entry point: where it is, how many bytes of it the call touches, what the call does with
// it, and whether a null pointer is refused (`need`). An entry point writes its arguments down once as a table of these
// (CallFrame in arima_runtime.cpp); the null check, the overlap rule and the staging of a host-buffer call all read it.
enum BufRole : uint8_t { kBufIn, kBufOut, kBufOptOut, kBufInOut };
struct Buf {
    const void *p;
    int64_t bytes;
    BufRole role;
    bool need;
    bool read() const { return role == kBufIn || role == kBufInOut; }
    bool written() const { return role != kBufIn; }
};
inline Buf buf_in(const void *p, int64_t bytes, bool need = true) { return {p, bytes, kBufIn, need}; }
inline Buf buf_out(void *p, int64_t bytes) { return {p, bytes, kBufOut, true}; }
inline Buf buf_opt_out(void *p, int64_t bytes) { return {p, bytes, kBufOptOut, false}; }   // null: not wanted
inline Buf buf_inout(void *p, int64_t bytes) { return {p, bytes, kBufInOut, true}; }
constexpr int kMaxBufs = 8;

inline bool missing_buffer(const Buf *t, int n) {
    for (int i = 0; i < n; ++i)
        if (t[i].need && !t[i].p) return true;
    return false;
}

// A table's two lists for find_overlap, in table order. Whatever the call writes is an output, an in-out buffer too:
// that the call also reads it adds nothing to what an output may not meet.
inline void split_spans(const Buf *t, int n, ByteSpan *in, int *n_in, ByteSpan *out, int *n_out) {
    *n_in = *n_out = 0;
    for (int i = 0; i < n; ++i)
        (t[i].written() ? out[(*n_out)++] : in[(*n_in)++]) = ByteSpan(t[i].p, t[i].bytes);
}
inline Overlap table_overlap(const Buf *t, int n) {
    ByteSpan in[kMaxBufs], out[kMaxBufs];
    int n_in, n_out;
    split_spans(t, n, in, &n_in, out, &n_out);
    return find_overlap(in, n_in, out, n_out);
}

// The (offset, length) pieces par_memcpy copies, one per thread: at most `threads` of them, none below 4 MiB unless
// it is the only one, every boundary a multiple of 64 bytes.
inline std::vector<std::pair<size_t, size_t>> memcpy_parts(size_t bytes, int threads) {
    std::vector<std::pair<size_t, size_t>> parts;
    const size_t min_part = size_t(4) << 20;
    const int t = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(threads, 1), bytes / min_part));
    if (t <= 1) {
        if (bytes) parts.emplace_back(size_t(0), bytes);
        return parts;
    }
    const size_t part = (bytes + t - 1) / t / 64 * 64 + 64;
    for (int i = 0; i < t; ++i) {
        const size_t off = (size_t)i * part;
        if (off >= bytes) break;
        parts.emplace_back(off, std::min(part, bytes - off));
    }
    return parts;
}

// memcpy with `threads` host threads (the caller's pageable rows into a pinned block: one thread copies at a fraction
// of the host's memory bandwidth, a PCIe Gen5 x16 link needs several)
inline void par_memcpy(void *dst, const void *src, size_t bytes, int threads) {
    const auto parts = memcpy_parts(bytes, threads);
    if (parts.size() <= 1) {
        if (bytes) memcpy(dst, src, bytes);
        return;
    }
    std::vector<std::thread> pool;
    for (const auto &pt : parts) {
        const size_t off = pt.first, len = pt.second;
        pool.emplace_back([=] { memcpy((char *)dst + off, (const char *)src + off, len); });
    }
    for (auto &th : pool) th.join();
}

// rows of one slice of a sliced device fit: whole thousands (1024) of rows of ld_doubles doubles within slice_bytes,
// at least 1024
inline int64_t fit_slice_rows(int64_t slice_bytes, int64_t ld_doubles) {
    return std::max<int64_t>(1024, slice_bytes / (ld_doubles * (int64_t)sizeof(double)) / 1024 * 1024);
}

// rows of one slice of the residual diagnostics: multiples of 64 rows within slice_bytes, at least 64
inline int64_t diag_slice_rows(int64_t slice_bytes, int64_t ld_doubles) {
    return std::max<int64_t>(64, slice_bytes / (ld_doubles * (int64_t)sizeof(double)) / 64 * 64);
}

// series of one slice of the design-matrix regressions (AutoregressionX, bgtest, bptest): whole blocks of 64 series
// whose workspaces of ws_doubles doubles per series fit slice_bytes, at least one block
inline int64_t regress_slice_rows(int64_t slice_bytes, int64_t ws_doubles) {
    return std::max<int64_t>(64, slice_bytes / (std::max<int64_t>(ws_doubles, 1) * (int64_t)sizeof(double)) / 64 * 64);
}

}  // namespace plan
}  // namespace sts
