// slot_walk.hpp -- the walk over the owned slots in slot order, shared by export.hip, potential.hip and remove.hip's
// removal by box (device-inline only).
//
// One workgroup of SLOT_THREADS walks a tile of SLOT_TILE slots (kernels.h): wave w of tile t holds the slots
// [t * SLOT_TILE + w * 64 * SLOT_ITEMS, + 64 * SLOT_ITEMS), 64 at a time, one to a lane.  A count pass leaves per tile how
// many slots a predicate chose; the pass behind it puts the chosen slots in slot order: tiles_before, wave_offset,
// lane_rank.  The launch boundary between the passes is the only ordering; no atomic decides a position.
// wave_offset and tile_order_sums hold LDS of their own and barriers: EVERY thread of the workgroup must reach the call (an
// early return before it may depend on the block index or on kernel arguments only).
#pragma once

#include "kernels_common.hpp"

namespace psamd {

constexpr int SLOT_THREADS = 256;
constexpr int SLOT_WAVES = SLOT_THREADS / 64;
constexpr int SLOT_ITEMS = SLOT_TILE / SLOT_THREADS;     // 16 batches of 64 slots per wave
static_assert(SLOT_ITEMS * SLOT_THREADS == SLOT_TILE, "a wave walks SLOT_ITEMS batches of 64 slots");

// Live: 0 <= cell < num_cells_global, what psamd_live_count counts; the mid-step encodings cell <= -2 are not live.
__device__ __forceinline__ bool slot_live(const DevParams &P, int c) { return c >= 0 && c < P.num_cells_global; }

// the lanes below the calling one that are set in a wave's ballot
__device__ __forceinline__ int lane_rank(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// the calling lane's first slot of tile t (its k-th: + 64 * k), and a slot's cell word (past the owned slots: free)
__device__ __forceinline__ int slot_first(int t, int wv, int lane) { return t * SLOT_TILE + wv * 64 * SLOT_ITEMS + lane; }
__device__ __forceinline__ int slot_cell(const DevParams &P, const int *__restrict__ cell, int i) { return i < P.slots_total ? cell[i] : -1; }

// The calling wave's share of the counts of the tiles before tile t (strided over the workgroup, then the wave's
// butterfly); wave_offset adds the waves' shares up.
__device__ __forceinline__ int tiles_before(const int *__restrict__ tile_count, int t)
{
    int before = 0;
    for (int i = threadIdx.x; i < t; i += SLOT_THREADS) before += tile_count[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) before += __shfl_xor(before, m);
    return before;
}

// Where the first chosen slot of wave wv goes: the tiles before (before: tiles_before's result) and the waves before it
// in the tile (n: what the wave chose).  Every thread of the workgroup calls; one barrier.
template <typename T>
__device__ __forceinline__ T wave_offset(int before, int n, int wv, int lane)
{
    __shared__ int s_before[SLOT_WAVES], s_n[SLOT_WAVES];
    if (lane == 0) { s_before[wv] = before; s_n[wv] = n; }
    __syncthreads();
    T at = 0;
    for (int w = 0; w < SLOT_WAVES; w++) at += s_before[w] + (w < wv ? s_n[w] : 0);
    return at;
}

// N fp64 sums over per-tile partials in tile index order, by one workgroup of SLOT_THREADS: thread k < N returns sum k
// (the others 0).  A serial chain per sum, so the same bits on every run for a given number of tiles.  The partials pass
// through LDS a round of SLOT_THREADS tiles at a time: take(t, v) -- called once per tile, by the thread that holds it in
// its round -- leaves tile t's N partials in v (and may keep what else it wants of the tile).
template <int N, typename Take>
__device__ __forceinline__ double tile_order_sums(int ntiles, Take take)
{
    __shared__ double s_sum[N][SLOT_THREADS + (N > 1 ? 1 : 0)];     // (+ 1: the sums' rows start in different banks)
    const int tid = threadIdx.x;
    double sum = 0.0;
    for (int base = 0; base < ntiles; base += SLOT_THREADS) {
        if (base + tid < ntiles) {
            double v[N];
            take(base + tid, v);
#pragma unroll
            for (int k = 0; k < N; k++) s_sum[k][tid] = v[k];
        }
        __syncthreads();
        if (tid < N) {
            const int m = min(SLOT_THREADS, ntiles - base);
            const double *v = s_sum[tid];
            int j = 0;
            for (; j + 8 <= m; j += 8) {               // eight reads in flight, then their adds in order
                double x[8];
#pragma unroll
                for (int i = 0; i < 8; i++) x[i] = v[j + i];
#pragma unroll
                for (int i = 0; i < 8; i++) sum += x[i];
            }
            for (; j < m; j++) sum += v[j];
        }
        __syncthreads();
    }
    return sum;
}

}  // namespace psamd
