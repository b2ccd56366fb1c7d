// nbr_walk.hpp -- psamd_neighbours' walk of one (own cell, 64-particle slice) task, shared by its count pass and its fill
// pass (neighbours.hip): the queries, the candidates, their order and the test are written once, here (device-inline only).
// include/psamd.h, "neighbours within a radius", holds the definition.
//
// A functor F sees the task through three calls, every lane of the wave making each:
//   f.begin(gi, valid)            the lane's query has sorted index gi (valid: the lane holds one)
//   f(hit, id, d2)                one candidate in walk order -- the same candidate for all lanes; hit: it is a neighbour of
//                                 the lane's query; id: its global slot id (wave-uniform); d2: the pair's squared distance
//   f.end(gi, valid)
// Candidates that are kids, that lie past a list's end or -- by sorted index -- are the lane's own entry never hit.
#pragma once

#include "pair_math.hpp"

namespace psamd {

// Eight bodies from jj on of one list (wave-uniform pointers: scalar loads of the x, y, z, age and id planes).  Only the first
// `rem` are bodies of the list: the others are read -- inside the buffers, which carry the slack -- and dropped.  SELF: the
// list is the lane's own cell's and body 0 has sorted index gj0.
// d2 is pairs_dist<8, false>'s: RN(RN(RN(rx rx) + RN(ry ry)) + RN(rz rz)) in packed fp32, nothing fused (-ffp-contract=off;
// neighbours.hip's header comment says how the ISA was checked).
template <bool SELF, typename F>
__device__ __forceinline__ void nbr_group(const PairCtx &ctx, const float *__restrict__ sx, const float *__restrict__ sy,
                                          const float *__restrict__ sz, const float *__restrict__ sage,
                                          const int *__restrict__ sid, int jj, int rem, int gj0, float kid_thr, float r2, F &f)
{
    constexpr int NQ = 8;
    v2f qx[NQ / 2], qy[NQ / 2], qz[NQ / 2];
#pragma unroll
    for (int i = 0; i < NQ / 2; i++) {
        qx[i] = v2f{sx[jj + 2 * i], sx[jj + 2 * i + 1]};
        qy[i] = v2f{sy[jj + 2 * i], sy[jj + 2 * i + 1]};
        qz[i] = v2f{sz[jj + 2 * i], sz[jj + 2 * i + 1]};
    }
    PairRows<NQ> r;
    pairs_dist<NQ, false>(ctx, qx, qy, qz, 0.f, r);
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        const float d2 = (i & 1) ? r.d[i >> 1].y : r.d[i >> 1].x;
        const bool body = i < rem && !(sage[jj + i] < kid_thr);         // a scalar condition: the body, not the lane
        bool hit = body && d2 <= r2;                                    // (a NaN on either side: no neighbour)
        if (SELF) hit = hit && gj0 + jj + i != ctx.gi;
        f(hit, sid[jj + i], d2);
    }
}

template <bool SELF, typename F>
__device__ __forceinline__ void nbr_list(const PairCtx &ctx, const float *__restrict__ snap_soa, size_t cap,
                                         const float *__restrict__ snap_age, const int *__restrict__ sorted_id, int nb, int n,
                                         float kid_thr, float r2, F &f)
{
    const float *sx = snap_soa + nb;
    for (int jj = 0; jj < n; jj += 8)
        nbr_group<SELF>(ctx, sx, sx + cap, sx + 2 * cap, snap_age + nb, sorted_id + nb, jj, n - jj, nb, kid_thr, r2, f);
}

// The calling wave's task: (cell, slice) tasks of every own cell, cell-major; four independent waves per workgroup, an XCD's
// workgroups a contiguous run of cells (potential.hip, k_pot_pairs).  A slice past its cell's count ends at once.
template <typename F>
__device__ __forceinline__ void nbr_walk_task(const DevParams &P, const int *__restrict__ cell_start,
                                              const float *__restrict__ snap_soa, const float *__restrict__ snap_age,
                                              const int *__restrict__ sorted_id, const float4 *__restrict__ pos4, float r2, F &f)
{
    const int lane = threadIdx.x & 63;
    const int ntask = P.n_own_cells * P.slices, nwg = (ntask + 3) >> 2;
    if ((int)blockIdx.x >= nwg) return;
    const int slot = __builtin_amdgcn_readfirstlane(xcd_contiguous(blockIdx.x, nwg) * 4 + (int)(threadIdx.x >> 6));
    if (slot >= ntask) return;
    const int c = slot / P.slices, slice = slot - c * P.slices;
    const int base = cell_start[c];
    const int cnt = min(cell_start[c + 1] - base, P.max_per_cell);
    const int first = slice * 64;
    if (first >= cnt) return;
    const bool valid = lane < min(64, cnt - first);
    const int gi = base + first + (valid ? lane : 0);
    const size_t cap = (size_t)P.sorted_cap;
    float mx = snap_soa[gi], my = snap_soa[cap + gi], mz = snap_soa[2 * cap + gi];
    if (snap_age[gi] < P.kid_thr) {              // a kid's snapshot position is the origin (grid.hip): its own is in its slot
        const int si = slot_index(P, sorted_id[gi]);
        if (si >= 0) { const float4 p = pos4[si]; mx = p.x; my = p.y; mz = p.z; }
    }
    int i1, i2, i3;
    cell_coords(P, c, i1, i2, i3);
    const PairCtx ctx = {mx, my, mz, 0.f, 0, gi, false};
    int my_nb, my_cnt;
    stencil_ranges(P, cell_start, i1, i2, i3, lane, my_nb, my_cnt);
    f.begin(gi, valid);
    nbr_list<true>(ctx, snap_soa, cap, snap_age, sorted_id, base, cnt, P.kid_thr, r2, f);      // the own cell first, as the stencil has it
    for (int k = 1; k < STENCIL; k++) {
        const int nb = __builtin_amdgcn_readlane(my_nb, k), n = __builtin_amdgcn_readlane(my_cnt, k);
        nbr_list<false>(ctx, snap_soa, cap, snap_age, sorted_id, nb, n, P.kid_thr, r2, f);
    }
    f.end(gi, valid);
}

}  // namespace psamd
