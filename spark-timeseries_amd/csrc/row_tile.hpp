// row_tile.hpp — the memory path of the one-lane-per-series streaming kernels (forecast, effects, diagnostics, the
// small models). One wave owns 64 rows (series) and walks them in [64 rows x CH steps] tiles:
//   load   CH coalesced loads (CH consecutive doubles of 64 / CH rows each) prefetch the next tile into registers
//   store  into a padded LDS array (row stride CH + 1 doubles: 64 lanes reading one column of their own rows spread
//          over the banks), which transposes the tile: each lane then steps through its own row
//   flush  an output that is final at its own step overwrites the input in LDS, and the tile leaves as coalesced row
//          segments at CH boundaries (two full 128-B lines per row for CH = 32 and 128-B aligned output rows)
// Nothing outside [0, N) x [0, T) is read or written. What a kernel carries across tile boundaries is its own.
#pragma once
#include <hip/hip_runtime.h>

namespace sts {

template <int CH>
struct RowTile {
    static constexpr int kWave = 64;
    static constexpr int RPL = kWave / CH;            // rows per coalesced load instruction
    static_assert(kWave % CH == 0, "tile width must divide the wave");
    typedef double Lds[kWave][CH + 1];

    // the lane-to-element mapping: load j of a lane is element col(lane) of row row(lane, j), stored at [row][col]
    static constexpr int col(int lane) { return lane % CH; }
    static constexpr int row(int lane, int j) { return j * RPL + lane / CH; }
    static constexpr bool covers_the_tile_once() {    // 64 lanes x CH loads: every (row, column) exactly once
        int seen[kWave][CH] = {};
        for (int lane = 0; lane < kWave; ++lane)
            for (int j = 0; j < CH; ++j) ++seen[row(lane, j)][col(lane)];
        for (int r = 0; r < kWave; ++r)
            for (int c = 0; c < CH; ++c)
                if (seen[r][c] != 1) return false;
        return true;
    }

    // bit r = row row0 + r is below N
    static __device__ __forceinline__ unsigned long long rows_below(int64_t row0, int64_t N) {
        const int64_t n = N - row0;
        return n >= kWave ? ~0ull : n <= 0 ? 0ull : (1ull << n) - 1ull;
    }

    // The tile of columns [cb, cb + CH) into registers, rows of `mask` (wave-uniform) only: pf[j] of the other rows is
    // left as it is. The column is clamped into [0, T) (a tile may start before 0 or end past T - 1; never consumed).
    static __device__ __forceinline__ void load(double (&pf)[CH], const double *in, int64_t ld, int64_t row0, int T,
                                                int64_t cb, int lane, unsigned long long mask) {
        const int64_t tt = cb + col(lane) < T ? cb + col(lane) : (int64_t)T - 1;
        int64_t first = (row0 + row(lane, 0)) * ld + (tt < 0 ? 0 : tt);
        // One base address and a uniform stride. The barrier keeps the CH row addresses from being formed once and
        // held (128 registers) across the pass: they are rebuilt from this one offset, one add each, at every tile.
        // It is on the offset, not the pointer, so that `in` stays known as global memory (a flat load would also
        // count on the LDS counter)
        asm volatile("" : "+v"(first));
        const double *src = in + first;
        const int64_t jstride = (int64_t)RPL * ld;
        if (mask == ~0ull) {
#pragma unroll
            for (int j = 0; j < CH; ++j) pf[j] = src[j * jstride];
        } else {
            unsigned long long mine = mask >> row(lane, 0);
            // likewise for the CH row predicates: held across the pass they are 2 CH scalar registers, which a kernel
            // that also holds its flush's row guards does not have (they would spill into vector lanes)
            asm volatile("" : "+v"(mine));
#pragma unroll
            for (int j = 0; j < CH; ++j)
                if ((mine >> (j * RPL)) & 1ull) pf[j] = src[j * jstride];
        }
    }

    static __device__ __forceinline__ void store(Lds &tile, const double (&pf)[CH], int lane) {
#pragma unroll
        for (int j = 0; j < CH; ++j) tile[row(lane, j)][col(lane)] = pf[j];
    }

    // columns [cb, cb + CH) below T of the rows below N, as coalesced row segments
    static __device__ __forceinline__ void flush(const Lds &tile, double *out, int64_t ld_out, int64_t row0, int64_t N,
                                                 int T, int cb, int lane) {
        const int idx = cb + col(lane);
        if (idx >= T) return;
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int r = row(lane, j);
            if (row0 + r < N) out[(row0 + r) * ld_out + idx] = tile[r][col(lane)];
        }
    }

    // One read-only pass over columns [0, T). body(cb, n): the lane's row is tile[lane][0 .. n), columns cb .. cb + n.
    template <class Body>
    static __device__ __forceinline__ void read(Lds &tile, const double *in, int64_t ld, int64_t row0, int T, int lane,
                                                unsigned long long mask, Body &&body) {
        if (T <= 0) return;
        double pf[CH] = {};
        load(pf, in, ld, row0, T, 0, lane, mask);
        for (int cb = 0; cb < T; cb += CH) {
            __syncthreads();                          // every lane is done with the last tile (and its flush)
            store(tile, pf, lane);
            __syncthreads();
            if (cb + CH < T) load(pf, in, ld, row0, T, cb + CH, lane, mask);
            body(cb, cb + CH < T ? CH : T - cb);
        }
    }

    // The same pass with an output: body leaves column cb + c of its row in tile[lane][c]; the tile is flushed once
    // every lane has written. `out` may be `in` with equal strides (no __restrict__): a wave reads a tile before it
    // writes it, the tile prefetched meanwhile covers disjoint columns, and a wave owns its rows.
    template <class Body>
    static __device__ __forceinline__ void map(Lds &tile, const double *in, int64_t ld_in, double *out, int64_t ld_out,
                                               int64_t row0, int64_t N, int T, int lane, unsigned long long mask,
                                               Body &&body) {
        read(tile, in, ld_in, row0, T, lane, mask, [&](int cb, int n) {
            body(cb, n);
            __syncthreads();
            flush(tile, out, ld_out, row0, N, T, cb, lane);
        });
    }
};

static_assert(RowTile<16>::covers_the_tile_once() && RowTile<32>::covers_the_tile_once(), "lane-to-element mapping");

}  // namespace sts
