// multisplit.hpp -- the deterministic stable multisplit of a tile of entries by queue record, shared by inject.hip and
// remove.hip, and the entry front they share with update.hip (device-inline only).
//
// A tile of ENTRY_TILE = SPLIT_THREADS * SPLIT_GROUPS entries is ranked by one workgroup of 16 waves; wave w holds the
// entries [(w * SPLIT_GROUPS + g) * 64, + 64), g = 0 .. SPLIT_GROUPS - 1, one to a lane.  An entry's key is its record (>= 0), or a negative
// number for an entry that takes no part.  The rank of an entry is the number of earlier entries of the tile with the
// same record: inside a group by ballot + mbcnt per distinct record, across groups by the waves taking turns in entry
// order at the tile's per-record counts.  No atomic decides an order: the result is the same on every run.
#pragma once

#include <climits>

#include "slot_walk.hpp"

namespace psamd {

constexpr int SPLIT_THREADS = 1024;
constexpr int SPLIT_WAVES = SPLIT_THREADS / 64;
constexpr int SPLIT_GROUPS = ENTRY_TILE / SPLIT_THREADS;
static_assert(SPLIT_GROUPS * SPLIT_THREADS == ENTRY_TILE, "a wave ranks SPLIT_GROUPS consecutive groups of 64 entries");
constexpr int SPLIT_LDS_RECORDS = 8192;       // records counted in LDS (32 KB); more: in the tile's row in global memory

// how many of the caller's max_count entries count: all, or what the device word says, clamped
__device__ __forceinline__ int entry_count(const int64_t *count_dev, int64_t max_count)
{
    if (!count_dev) return (int)max_count;
    const int64_t v = *count_dev;
    return (int)(v < 0 ? 0 : v > max_count ? max_count : v);
}
__device__ __forceinline__ int entry_tiles(int n) { return (int)(((int64_t)n + ENTRY_TILE - 1) / ENTRY_TILE); }

// An entry that names a slot by its id (remove.hip, update.hip): the storage index of the slot if the entry can act on it
// (valid id, owned, live now), else -1 - outcome.  The three outcomes are the same numbers in both services' headers.
enum { ID_NOT_LIVE = 1, ID_FOREIGN = 2, ID_INVALID = 3 };
__device__ __forceinline__ int remove_classify(const DevParams &P, int id, const int *__restrict__ cell)
{
    if (id < 0 || id >= P.container) return -1 - ID_INVALID;
    const int si = slot_index(P, id);
    if (si < 0) return -1 - ID_FOREIGN;
    return slot_live(P, cell[si]) ? si : -1 - ID_NOT_LIVE;
}

// a lane's rank among the group's lanes of the same record, the group's count of that record and the lane that will
// account for it (the lowest)
__device__ __forceinline__ void split_group_rank(int r, int lane, int &in_rank, int &pop, int &lead)
{
    in_rank = 0; pop = 0; lead = lane;
    unsigned long long todo = __ballot(r >= 0);
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        const int r0 = __builtin_amdgcn_readlane(r, l);
        const unsigned long long m = __ballot(r == r0);
        if (r == r0) {
            in_rank = lane_rank(m);
            pop = __popcll(m);
            lead = l;
        }
        todo &= ~m;
    }
}

// the waves take turns in entry order; a group's lowest lane of each record takes the record's running count
// (leaders of one group hold distinct records; a wave's groups follow one another).  cnt: the tile's per-record counts,
// zeroed by the caller, in LDS or -- GLOBAL -- in the tile's row in global memory.  All threads of the workgroup call.
template <int GROUPS, bool GLOBAL>
__device__ __forceinline__ void split_take_turns(const int (&rec)[GROUPS], const int (&in_rank)[GROUPS], const int (&pop)[GROUPS],
                                                 const int (&lead)[GROUPS], int *cnt, int wave, int lane, int (&at)[GROUPS])
{
    for (int w = 0; w < SPLIT_WAVES; w++) {
        if (wave == w) {
#pragma unroll
            for (int g = 0; g < GROUPS; g++) {
                int b = 0;
                if (rec[g] >= 0 && lead[g] == lane) b = atomicAdd(&cnt[rec[g]], pop[g]);
                at[g] = __shfl(b, lead[g]) + in_rank[g];
            }
        }
        if (GLOBAL) __threadfence();
        __syncthreads();
    }
}

// The front of a tile's workgroup (LDS: nrec <= SPLIT_LDS_RECORDS, launched with nrec words of dynamic LDS, lds_cnt),
// around the kernel's own loop over its groups, which fills a SplitKeys: every entry's key and split_group_rank's results.
//   split_tile_begin  the tile's counts zeroed (its barrier also covers what the kernel initialised in LDS just before)
//   split_tile_store  the waves' turns; ent[i] = (key, rank in the tile); the counts to the tile's row of tcount
struct SplitKeys { int rec[SPLIT_GROUPS], in_rank[SPLIT_GROUPS], pop[SPLIT_GROUPS], lead[SPLIT_GROUPS], *cnt; };

// entry of the calling lane in group g of its wave, tile t
__device__ __forceinline__ int split_entry(int t, int g) { return t * ENTRY_TILE + (((int)threadIdx.x >> 6) * SPLIT_GROUPS + g) * 64 + ((int)threadIdx.x & 63); }

template <bool LDS>
__device__ __forceinline__ void split_tile_begin(int t, int nrec, int *lds_cnt, int *__restrict__ tcount, SplitKeys &k)
{
    k.cnt = LDS ? lds_cnt : tcount + (size_t)t * nrec;
    for (int r = (int)threadIdx.x; r < nrec; r += SPLIT_THREADS) k.cnt[r] = 0;
    if (!LDS) __threadfence();
    __syncthreads();
}

template <bool LDS>
__device__ __forceinline__ void split_tile_store(int t, int n, int nrec, const SplitKeys &k, int2 *__restrict__ ent, int *__restrict__ tcount)
{
    const int tid = (int)threadIdx.x;
    int at[SPLIT_GROUPS];
    split_take_turns<SPLIT_GROUPS, !LDS>(k.rec, k.in_rank, k.pop, k.lead, k.cnt, tid >> 6, tid & 63, at);
#pragma unroll
    for (int g = 0; g < SPLIT_GROUPS; g++) {
        const int i = split_entry(t, g);
        if (i < n) ent[i] = make_int2(k.rec[g], k.rec[g] >= 0 ? at[g] : 0);
    }
    if (LDS) for (int r = tid; r < nrec; r += SPLIT_THREADS) tcount[(size_t)t * nrec + r] = k.cnt[r];
}

// one record's exclusive prefix of the tiles' counts, in tile order, in place; returns the record's total
__device__ __forceinline__ int split_tile_prefix(int *__restrict__ tcount, int nrec, int tiles, int r)
{
    int run = 0;
    for (int t = 0; t < tiles; t++) {
        int *p = tcount + (size_t)t * nrec + r;
        const int c = *p;
        *p = run;
        run += c;
    }
    return run;
}

// sums `v` over the workgroup (int64, order-independent) into out; s: one word of LDS per value, zeroed here
template <int N>
__device__ __forceinline__ void block_sum(const long long (&v)[N], unsigned long long *s, long long (&out)[N])
{
    if (threadIdx.x < N) s[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) {
        long long x = v[k];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
        if ((threadIdx.x & 63) == 0 && x) atomicAdd(&s[k], (unsigned long long)x);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) out[k] = (long long)s[k];
}

// a call's result record: into the context's own, and into the caller's if it gave one
template <typename R>
__device__ __forceinline__ void write_result(R *own, R *out, const R &res)
{
    *own = res;
    if (out && out != own) *out = res;
}

}  // namespace psamd
