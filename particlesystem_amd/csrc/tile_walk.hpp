// tile_walk.hpp -- the force walks that take their bodies through LDS tiles (force.hip's k_pairs_balanced):
// pairs_task_tile for a wave with its SIMD (almost) to itself, merged_pack_task for the packs of partly filled slices
#pragma once

#include "balanced.hpp"
#include "pair_math.hpp"

namespace psamd {

constexpr int MERGE_TILE = 4 * 64 + 4;          // floats per lane group: x[64] y[64] z[64] w[64] + skew

// The same walk for a wave that has its SIMD (almost) to itself -- a slab of a multi-GPU run has
// about 1.5 force tasks per SIMD.  There the scalar-load walk of force.hip's pairs_task is latency-bound (one
// wave cannot cover its own s_load round trips: 1.6x slower per task, the sweep of the wave
// count in DESIGN.md), so the bodies come as 64-body tiles instead: one vector load per lane, issued a
// whole tile ahead (vector loads retire in order, so they pipeline), through LDS (SoA, no
// barrier: a wave reads only its own tiles and its LDS operations complete in order), read back
// as broadcast 16-byte rows.  Same arithmetic, same order: short last tiles are padded with
// massless bodies far outside the box (r * 0 = +-0 added to a sum that started at +0 changes
// nothing, as for kids).  Two-pass mode only (flags are settled), lean arithmetic.
//
// A wave serves up to four lane GROUPS, each a run of one cell's particles with its own stencil
// and its own tile (the groups' tiles skewed by 16 bytes onto different banks): one group of up
// to 64 lanes = an ordinary (cell, slice) task; several = the partly filled last slices of up to
// four cells packed into one wave (a cell's list of ~148 particles fills two slices and a third
// of another).  All groups walk stencil step k together, tile by tile, for as many rows as the
// longest of their lists.
// (The two walks below still write their set-up twice.  Hoisting it was tried piece by piece against the generated code of
// k_pairs_balanced -- whose instances sit at 256 VGPRs and at 71 VGPRs for seven waves per SIMD -- and only the tile
// store came out unchanged; the lane -> group mapping, the range table with its read-out, the LDS group read in the pack
// walk and the pack -> TileGroups conversion each moved instructions or registers: profiles/pairs_split_isa.txt.)
struct TileGroups {
    int ng;
    int cell[4], first[4], count[4];      // group g: particles active_list[cell_start[cell] + first ..][0 .. count)
};

// this lane's body of group gg's tile (SoA, the groups' tiles skewed by 16 bytes)
__device__ __forceinline__ void store_tile_body(float *tile, int gg, const float4 v)
{
    float *t = tile + gg * MERGE_TILE + (threadIdx.x & 63);
    t[0] = v.x; t[64] = v.y; t[128] = v.z; t[192] = v.w;
}

// NG: how many groups the code is built for (1: an ordinary task, nothing per-group left in it; 4: a pack)
template <int MODE, int NQ, int NG, bool ONE_T>
__device__ __forceinline__ void pairs_task_tile(const DevParams &P, const int *__restrict__ cell_start,
                                                const SnapSoa snap4, const ForceBuf force4,
                                                const TileGroups &G, float *tile, const int *__restrict__ active_list,
                                                int k0, int k1, int *ready, FrameScalars *fs)
{
    const int lane = threadIdx.x & 63;
    int off[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < 4; g++) off[g + 1] = off[g] + ((g < NG && g < G.ng) ? G.count[g] : 0);
    const int g = NG == 1 ? 0 : (lane >= off[1]) + (lane >= off[2]) + (lane >= off[3]);       // a lane past the last group: 3, invalid
    const bool valid = lane < off[4];
    const int gc = valid ? (g == 0 ? G.cell[0] : g == 1 ? G.cell[1] : g == 2 ? G.cell[2] : G.cell[3]) : G.cell[0];
    const int gf = valid ? (g == 0 ? G.first[0] : g == 1 ? G.first[1] : g == 2 ? G.first[2] : G.first[3]) : G.first[0];
    const int l = valid ? lane - (g == 0 ? off[0] : g == 1 ? off[1] : g == 2 ? off[2] : off[3]) : 0;
    const int gi = active_list[cell_start[gc] + gf + l];
    const float4 me = snap4[gi];
    const float eps2f = (float)P.eps2;
    // neighbour ranges of all groups: entry e = group * 27 + stencil step, held by lane e % 64
    int tab_nb[2] = {0, 0}, tab_cnt[2] = {0, 0};
#pragma unroll
    for (int r = 0; r < (NG == 1 ? 1 : 2); r++) {
        const int e = lane + 64 * r, eg = e / STENCIL, ek = e - eg * STENCIL;
        const int ec = (eg < NG && eg < G.ng) ? (eg == 0 ? G.cell[0] : eg == 1 ? G.cell[1] : eg == 2 ? G.cell[2] : G.cell[3]) : -1;
        if (ec >= 0) {
            int i1, i2, i3;
            cell_coords(P, ec, i1, i2, i3);
            const int nc = local_cell(P, i3 + c_stencil[ek][2], i1 + c_stencil[ek][1], i2 + c_stencil[ek][0]);
            if (nc >= 0) {
                tab_nb[r] = cell_start[nc];
                tab_cnt[r] = min(cell_start[nc + 1] - tab_nb[r], P.max_per_cell);
            }
        }
    }
    float ax = 0.f, ay = 0.f, az = 0.f;
    int flag = 0;
    const PairCtx ctx = {me.x, me.y, me.z, 0.f, 0, gi, false};
    if (k0 > 0 && !handoff_consume(force4 + gi, ax, ay, az, flag, valid, ready, k0)) {
        if (lane == 0) atomicOr(&fs->error, ERR_HANDOFF_TIMEOUT);
    }
    const float far = 1.0e6f;                                       // padding body, mass 0
    const float *tx = tile + (valid ? g : 0) * MERGE_TILE, *ty = tx + 64, *tz = tx + 128, *tw = tx + 192;
    int nbs[4] = {0, 0, 0, 0}, cnts[4] = {0, 0, 0, 0};
    // ranges of stencil step k for every group; returns the longest list
    auto step_ranges = [&](int k) -> int {
        int longest = 0;
#pragma unroll
        for (int gg = 0; gg < NG; gg++) {
            const int e = gg * STENCIL + k;
            nbs[gg] = __builtin_amdgcn_readlane(e < 64 ? tab_nb[0] : tab_nb[1], e & 63);
            cnts[gg] = gg < G.ng ? __builtin_amdgcn_readlane(e < 64 ? tab_cnt[0] : tab_cnt[1], e & 63) : 0;
            longest = max(longest, cnts[gg]);
        }
        return longest;
    };
    float4 pre[NG];
    auto fetch = [&](int t0) {                                      // this lane's body of every group's tile at row t0
#pragma unroll
        for (int gg = 0; gg < NG; gg++) {
            pre[gg] = make_float4(far, far, far, 0.f);
            if (gg < G.ng && lane < cnts[gg] - t0) pre[gg] = snap4[nbs[gg] + t0 + lane];
        }
    };
    // first non-empty step from k0 on, its first tiles fetched ahead
    int k = k0, t0 = 0, longest = 0;
    while (k < k1 && (longest = step_ranges(k)) == 0) k++;
    bool have = k < k1;
    if (have) fetch(0);
    while (have) {
        const int n = (min(64, longest - t0) + NQ - 1) & ~(NQ - 1);
        PS_WAVE_SYNC();                               // previous tiles fully consumed
#pragma unroll
        for (int gg = 0; gg < NG; gg++)
            if (gg < G.ng) store_tile_body(tile, gg, pre[gg]);
        PS_WAVE_SYNC();
        t0 += 64;                                     // advance to the next non-empty row of tiles
        if (t0 >= longest) {
            t0 = 0; longest = 0; k++;
            while (k < k1 && (longest = step_ranges(k)) == 0) k++;
        }
        have = k < k1;
        // issued after the fences (they drain outstanding loads), consumed a tile later
        if (have) fetch(t0);
        float dmin = 3.0e38f;
        // The tile's groups of NQ bodies, the NEXT group's LDS reads in flight while the current one is worked through
        // (this walk runs one or two waves to a SIMD: nobody else covers a read's round trip, and with all eight
        // reads followed at once by s_waitcnt lgkmcnt(0) a quarter of the loop was that wait).  Two register sets,
        // used in turn: LDS reads return in order, so the wait before a group is for that group's reads only.
        struct Group { v2f qx[NQ / 2], qy[NQ / 2], qz[NQ / 2], qw[NQ / 2]; };
        auto read_group = [&](int jj, Group &g) {               // 16-byte LDS reads, NQ is a multiple of 4
#pragma unroll
            for (int i = 0; i < NQ / 2; i += 2) {
                const float4 vx = *reinterpret_cast<const float4 *>(tx + jj + 2 * i);
                const float4 vy = *reinterpret_cast<const float4 *>(ty + jj + 2 * i);
                const float4 vz = *reinterpret_cast<const float4 *>(tz + jj + 2 * i);
                const float4 vw = *reinterpret_cast<const float4 *>(tw + jj + 2 * i);
                g.qx[i] = v2f{vx.x, vx.y}; g.qx[i + 1] = v2f{vx.z, vx.w};
                g.qy[i] = v2f{vy.x, vy.y}; g.qy[i + 1] = v2f{vy.z, vy.w};
                g.qz[i] = v2f{vz.x, vz.y}; g.qz[i + 1] = v2f{vz.z, vz.w};
                g.qw[i] = v2f{vw.x, vw.y}; g.qw[i + 1] = v2f{vw.z, vw.w};
            }
        };
        auto work_group = [&](const Group &g) {
            if (MODE == 1)
                pairsN_exact_lean<NQ, ONE_T>(P, ctx, g.qx, g.qy, g.qz, g.qw, 0, nullptr, nullptr, ax, ay, az, flag);
            else
                dmin = fminf(dmin, pairsN_fast<NQ>(ctx, g.qx, g.qy, g.qz, g.qw, eps2f, ax, ay, az));
        };
        Group a, b;
        read_group(0, a);
        for (int jj = 0; jj < n; jj += 2 * NQ) {
            if (jj + NQ < n) read_group(jj + NQ, b);
            work_group(a);
            if (jj + NQ < n) {
                if (jj + 2 * NQ < n) read_group(jj + 2 * NQ, a);
                work_group(b);
            }
        }
    }
    if (k1 < STENCIL) { handoff_publish(force4 + gi, ax, ay, az, flag, valid, ready, k1); return; }
    if (valid) force4.put(P, gc, gi, make_float4(ax, ay, az, __int_as_float(flag)));
}

// Merged task of the two-pass force pass: the partly filled last slices of up to four cells
// share one wave, each cell's particles in their own run of lanes.  Every lane group has its
// own stencil, so the bodies cannot come as scalar operands here: each group's current 64
// bodies sit in its own LDS tile (SoA, the groups' tiles skewed by 16 bytes so that they use
// different banks -- scripts/microbench/lds_groups.hip) and a lane reads its group's tile.
// All groups walk stencil step k together, tile by tile, for as many rows as the longest of
// their lists; shorter lists are padded with massless bodies far outside the box: such a
// row adds r * 0 = +-0 to a sum that started at +0 (bit-identical, as for kids).  Walked by the
// first workgroups of the balanced pass (WALK 0), beside its ordinary tasks.
template <int MODE, int NQ>
__device__ __forceinline__ void merged_pack_task(const DevParams &P, const int *__restrict__ cell_start,
                                                 const SnapSoa snap4,
                                                 const int *__restrict__ active_list,
                                                 const int *__restrict__ active_count,
                                                 const int4 *__restrict__ merged_tasks,
                                                 const ForceBuf force4, int slot, float *tile, WavePace &pace)
{
    const int lane = threadIdx.x & 63;
    // (Raising these waves' issue priority -- they run one per SIMD among six of the balanced
    // pass -- was tried: s_setprio(3) ended them 0.6 ms earlier and the
    // balanced pass 0.5 ms later, 2.26 -> 2.48 ms for the stage.)
    const int4 pk = merged_tasks[slot];
    const int cells[4] = {pk.x, pk.y, pk.z, pk.w};
    // lane ranges of the groups
    int off[5] = {0, 0, 0, 0, 0}, ng = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int r = cells[k] >= 0 ? (active_count[cells[k]] & 63) : 0;
        off[k + 1] = off[k] + r;
        if (cells[k] >= 0) ng = k + 1;
    }
    const int g = (lane >= off[1]) + (lane >= off[2]) + (lane >= off[3]);       // a lane past the last group: 3, invalid
    const bool valid = lane < off[4];
    const int c = valid ? (g == 0 ? cells[0] : g == 1 ? cells[1] : g == 2 ? cells[2] : cells[3]) : cells[0];
    const int l = valid ? lane - (g == 0 ? off[0] : g == 1 ? off[1] : g == 2 ? off[2] : off[3]) : 0;
    const int gi = active_list[cell_start[c] + (active_count[c] & ~63) + l];
    const float4 me = snap4[gi];
    const float eps2f = (float)P.eps2;

    // neighbour ranges of all groups: entry e = group * 27 + stencil step, held by lane e % 64
    int tab_nb[2] = {0, 0}, tab_cnt[2] = {0, 0};
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int e = lane + 64 * r, eg = e / 27, ek = e - eg * 27;
        const int ec = eg == 0 ? cells[0] : eg == 1 ? cells[1] : eg == 2 ? cells[2] : eg == 3 ? cells[3] : -1;
        if (ec >= 0) {
            int i1, i2, i3;
            cell_coords(P, ec, i1, i2, i3);
            const int nc = local_cell(P, i3 + c_stencil[ek][2], i1 + c_stencil[ek][1], i2 + c_stencil[ek][0]);
            if (nc >= 0) {
                tab_nb[r] = cell_start[nc];
                tab_cnt[r] = min(cell_start[nc + 1] - tab_nb[r], P.max_per_cell);
            }
        }
    }
    const float *tx = tile + (valid ? g : 0) * MERGE_TILE, *ty = tx + 64, *tz = tx + 128, *tw = tx + 192;
    const float far = 1.0e6f;                                       // padding body, mass 0
    const PairCtx ctx = {me.x, me.y, me.z, 0.f, 0, gi, false};
    float ax = 0.f, ay = 0.f, az = 0.f;
    int flag = 0;
    for (int k = 0; k < 27; k++) {
        int nbs[4], cnts[4], longest = 0;
#pragma unroll
        for (int gg = 0; gg < 4; gg++) {
            const int e = gg * 27 + k;
            nbs[gg] = __builtin_amdgcn_readlane(e < 64 ? tab_nb[0] : tab_nb[1], e & 63);
            cnts[gg] = gg < ng ? __builtin_amdgcn_readlane(e < 64 ? tab_cnt[0] : tab_cnt[1], e & 63) : 0;
            longest = max(longest, cnts[gg]);
        }
        for (int t0 = 0; t0 < longest; t0 += 64) {
            PS_WAVE_SYNC();                                         // previous tiles fully consumed
#pragma unroll
            for (int gg = 0; gg < 4; gg++) {
                if (gg < ng) {
                    float4 v = make_float4(far, far, far, 0.f);
                    if (lane < cnts[gg] - t0) v = snap4[nbs[gg] + t0 + lane];
                    store_tile_body(tile, gg, v);
                }
            }
            PS_WAVE_SYNC();
            const int n = (min(64, longest - t0) + NQ - 1) & ~(NQ - 1);
            float dmin = 3.0e38f;
            for (int jj = 0; jj < n; jj += NQ) {
                v2f qx[NQ / 2], qy[NQ / 2], qz[NQ / 2], qw[NQ / 2];   // 16-byte LDS reads, NQ is a multiple of 4
#pragma unroll
                for (int i = 0; i < NQ / 2; i += 2) {
                    const float4 vx = *reinterpret_cast<const float4 *>(tx + jj + 2 * i);
                    const float4 vy = *reinterpret_cast<const float4 *>(ty + jj + 2 * i);
                    const float4 vz = *reinterpret_cast<const float4 *>(tz + jj + 2 * i);
                    const float4 vw = *reinterpret_cast<const float4 *>(tw + jj + 2 * i);
                    qx[i] = v2f{vx.x, vx.y}; qx[i + 1] = v2f{vx.z, vx.w};
                    qy[i] = v2f{vy.x, vy.y}; qy[i + 1] = v2f{vy.z, vy.w};
                    qz[i] = v2f{vz.x, vz.y}; qz[i + 1] = v2f{vz.z, vz.w};
                    qw[i] = v2f{vw.x, vw.y}; qw[i + 1] = v2f{vw.z, vw.w};
                }
                if (MODE == 1)
                    pairsN_exact_lean<NQ>(P, ctx, qx, qy, qz, qw, 0, nullptr, nullptr, ax, ay, az, flag);
                else
                    dmin = fminf(dmin, pairsN_fast<NQ>(ctx, qx, qy, qz, qw, eps2f, ax, ay, az));
            }
        }
        pace.step();
    }
    if (valid) force4.put(P, c, gi, make_float4(ax, ay, az, 0.f));
}

}  // namespace psamd
