// multisplit.hpp -- the deterministic stable multisplit of a tile of entries by queue record, shared by inject.hip and
// remove.hip (device-inline only).
//
// A tile of SPLIT_THREADS * GROUPS entries is ranked by one workgroup of 16 waves; wave w holds the entries
// [(w * GROUPS + g) * 64, + 64), g = 0 .. GROUPS - 1, one to a lane.  An entry's key is its record (>= 0), or a negative
// number for an entry that takes no part.  The rank of an entry is the number of earlier entries of the tile with the
// same record: inside a group by ballot + mbcnt per distinct record, across groups by the waves taking turns in entry
// order at the tile's per-record counts.  No atomic decides an order: the result is the same on every run.
#pragma once

#include "kernels_common.hpp"

namespace psamd {

constexpr int SPLIT_THREADS = 1024;
constexpr int SPLIT_WAVES = SPLIT_THREADS / 64;

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
            in_rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
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

}  // namespace psamd
