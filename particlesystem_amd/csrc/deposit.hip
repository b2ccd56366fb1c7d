// deposit.hip -- psamd_deposit: the mass density of the frame on a regular lattice, cloud-in-cell, gathered on the device.
//
// Not part of the step and not in the reference.  The lattice has k = refine voxels per cell edge
// (M = G k per axis); a body spreads its mass |w_eff| over the (up to) eight voxels whose centres surround it, with the
// trilinear weights of include/psamd.h ("mass on a lattice").  The bodies are sorted by cell, so a voxel is GATHERED: every
// body that can reach it lies in the 27-cell stencil of the voxel's cell, and the voxel's value is formed by one wave from
// those lists in a fixed order -- no atomic touches a floating-point word, and a slab forms each voxel on one rank.
// Two launches that nothing in between has to wait for:
//   k_deposit<K>      one wave per task = (compute cell, block of at most 2 x 2 x 2 voxels of it): 1, 1 or 8 tasks a cell for
//                     K = 1, 2, 4; four independent waves per workgroup, an XCD's workgroups a contiguous run of tasks
//                     (force.hip, k_pairs).  The 27 list ranges come from stencil_ranges, in the reference's order; lane l
//                     takes entries l, l + 64, ... of every list (coalesced loads of the four snap_soa planes), forms the
//                     body's n0 and f once per axis and adds its terms to one fp64 accumulator per voxel of the block, all
//                     from +0.  A butterfly (lane l adds lane l ^ 32, then ^ 16 ... ^ 1) closes each accumulator; lane v
//                     stores voxel v as (float).  The task's partials -- the voxel sums added in voxel order, the largest
//                     float, and (a cell's first task, from the own cell's list) the finite and the skipped bodies -- meet
//                     the other three waves' in LDS and leave as the workgroup's one DepositPart, merged in task order.
//   k_deposit_finish  one workgroup: mass over the parts in task order (tile_order_sums: one serial fp64 chain), vmax and
//                     the counts; the context's own record and the caller's.
// A voxel's association therefore depends on the voxel and on the lists' lengths alone: not on the launch, the rank or the
// plan.  Terms are non-negative (weights in [0, 1], m = |w_eff|), a term whose weight is zero on some axis is +0 and adding
// it changes nothing, so every body of the stencil is simply added: the stencil rule of the header is the gather itself.
//
// VGPRs / waves per SIMD as the compiler reports them for gfx950, no instance with scratch, no LDS beyond the 96 bytes of
// the partials:    K = 1: 29 / 8      K = 2: 52 / 8      K = 4: 52 / 8      k_deposit_finish: 28 / 8 (its LDS: tile_order_sums')
#include "lattice.hpp"
#include "slot_walk.hpp"

namespace psamd {

constexpr int DEP_THREADS = 64 * DEPOSIT_WG_TASKS;
static_assert(DEP_THREADS == SLOT_THREADS, "k_deposit_finish is a workgroup of tile_order_sums");

// (the weights of one axis of one body: DepAxis, lattice.hpp -- psamd_sample reads a lattice back with the same ones)

template <int K>
__global__ __launch_bounds__(DEP_THREADS) void k_deposit(DevParams P, const int *__restrict__ cell_start,
                                                         const float *__restrict__ snap_soa, const DepositArgs a,
                                                         DepositPart *__restrict__ parts)
{
    constexpr int TPC = K == 4 ? 8 : 1, VB = K == 1 ? 1 : 2, NV = VB * VB * VB;
    __shared__ DepositPart s_part[DEPOSIT_WG_TASKS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ntask = comp_count(P) * TPC, nwg = (ntask + DEPOSIT_WG_TASKS - 1) / DEPOSIT_WG_TASKS;
    if ((int)blockIdx.x >= nwg) return;
    const int group = __builtin_amdgcn_readfirstlane(xcd_contiguous(blockIdx.x, nwg));
    const int task = group * DEPOSIT_WG_TASKS + wv;
    DepositPart mine;
    mine.mass = 0.0; mine.vmax = -__int_as_float(0x7f800000); mine.bodies = 0; mine.skipped = 0; mine.pad = 0;
    if (task < ntask) {
        const int c = comp_cell(P, task / TPC), blk = task % TPC;
        int i1, i2, i3;
        cell_coords(P, c, i1, i2, i3);               // (global coordinates, on a slab too)
        const int b1 = i1 * K + ((blk >> 1) & 1) * 2, b2 = i2 * K + (blk & 1) * 2, b3 = i3 * K + (blk >> 2) * 2;
        int my_nb, my_cnt;
        stencil_ranges(P, cell_start, i1, i2, i3, lane, my_nb, my_cnt);
        const size_t cap = (size_t)P.sorted_cap;
        double acc[NV];
#pragma unroll
        for (int v = 0; v < NV; v++) acc[v] = 0.0;
        int bodies = 0, skipped = 0;
        for (int k = 0; k < STENCIL; k++) {           // the stencil, in the reference's order; k == 0: the own cell
            const int nb = __builtin_amdgcn_readlane(my_nb, k), n = __builtin_amdgcn_readlane(my_cnt, k);
            const float *sx = snap_soa + nb;
            for (int e = lane; e < n; e += 64) {
                const float x = sx[e], y = sx[cap + e], z = sx[2 * cap + e], w = sx[3 * cap + e];
                const bool fin = dep_finite(x) && dep_finite(y) && dep_finite(z) && dep_finite(w);
                if (k == 0 && blk == 0) { if (fin) bodies++; else skipped++; }
                if (!fin) continue;
                const float m = fabsf(w);
                const DepAxis a1(-y, a), a2(x, a), a3(-z, a);
                float w1[VB], w2[VB], w3[VB];
#pragma unroll
                for (int v = 0; v < VB; v++) { w1[v] = a1.at(b1 + v); w2[v] = a2.at(b2 + v); w3[v] = a3.at(b3 + v); }
#pragma unroll
                for (int v3 = 0; v3 < VB; v3++)
#pragma unroll
                    for (int v1 = 0; v1 < VB; v1++)
#pragma unroll
                        for (int v2 = 0; v2 < VB; v2++)
                            acc[(v3 * VB + v1) * VB + v2] += (double)__fmul_rn(__fmul_rn(__fmul_rn(w1[v1], w2[v2]), w3[v3]), m);
            }
        }
        // a butterfly per voxel: the same fixed tree on every run (PotAcc::wave_reduce, potential.hip)
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) {
#pragma unroll
            for (int v = 0; v < NV; v++) acc[v] += __shfl_xor(acc[v], sh);
            bodies += __shfl_xor(bodies, sh); skipped += __shfl_xor(skipped, sh);
        }
        const int64_t M = a.M;
#pragma unroll
        for (int v3 = 0; v3 < VB; v3++)
#pragma unroll
            for (int v1 = 0; v1 < VB; v1++)
#pragma unroll
                for (int v2 = 0; v2 < VB; v2++) {
                    const int v = (v3 * VB + v1) * VB + v2;
                    const float val = (float)acc[v];
                    if (lane == v) a.out[((int64_t)(b3 + v3) * M + (b1 + v1)) * M + (b2 + v2)] = val;
                    mine.mass += acc[v];
                    mine.vmax = fmaxf(mine.vmax, val);
                }
        mine.bodies = bodies; mine.skipped = skipped;
    }
    if (lane == 0) s_part[wv] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        DepositPart p = s_part[0];
        for (int w = 1; w < DEPOSIT_WG_TASKS; w++) {
            p.mass += s_part[w].mass; p.vmax = fmaxf(p.vmax, s_part[w].vmax);
            p.bodies += s_part[w].bodies; p.skipped += s_part[w].skipped;
        }
        parts[group] = p;
    }
}

__global__ __launch_bounds__(DEP_THREADS) void k_deposit_finish(int nparts, int64_t voxels, const DepositPart *__restrict__ parts,
                                                                psamd_deposit_result *__restrict__ own,
                                                                psamd_deposit_result *__restrict__ out)
{
    __shared__ float s_vmax[DEPOSIT_WG_TASKS];
    __shared__ long long s_bodies[DEPOSIT_WG_TASKS], s_skipped[DEPOSIT_WG_TASKS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float vmax = -__int_as_float(0x7f800000);
    long long bodies = 0, skipped = 0;
    const double mass = tile_order_sums<1>(nparts, [&](int t, double (&v)[1]) {
        const DepositPart p = parts[t];
        v[0] = p.mass;
        vmax = fmaxf(vmax, p.vmax); bodies += p.bodies; skipped += p.skipped;
    });
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        vmax = fmaxf(vmax, __shfl_xor(vmax, sh)); bodies += __shfl_xor(bodies, sh); skipped += __shfl_xor(skipped, sh);
    }
    if (lane == 0) { s_vmax[wv] = vmax; s_bodies[wv] = bodies; s_skipped[wv] = skipped; }
    __syncthreads();
    if (tid == 0) {
        psamd_deposit_result r;
        r.voxels = voxels; r.bodies = 0; r.skipped = 0; r.mass = mass; r.vmax = (double)s_vmax[0];
        for (int w = 0; w < DEPOSIT_WG_TASKS; w++) {
            r.bodies += s_bodies[w]; r.skipped += s_skipped[w]; r.vmax = fmax(r.vmax, (double)s_vmax[w]);
        }
        *own = r;
        if (out) *out = r;
    }
}

hipError_t launch_deposit(hipStream_t st, const DevParams &P, const DeviceState &d, const DepositArgs &a, const DepositScratch &s)
{
    const int K = a.refine, ncomp = comp_count(P), ntask = ncomp * deposit_cell_tasks(K);
    const int nwg = (ntask + DEPOSIT_WG_TASKS - 1) / DEPOSIT_WG_TASKS;
    if (nwg > 0) {
        if (K == 1) k_deposit<1><<<nwg, DEP_THREADS, 0, st>>>(P, d.cell_start, d.snap_soa, a, s.parts);
        else if (K == 2) k_deposit<2><<<nwg, DEP_THREADS, 0, st>>>(P, d.cell_start, d.snap_soa, a, s.parts);
        else k_deposit<4><<<nwg, DEP_THREADS, 0, st>>>(P, d.cell_start, d.snap_soa, a, s.parts);
        PS_LAUNCH_CHECK();
    }
    k_deposit_finish<<<1, DEP_THREADS, 0, st>>>(nwg, (int64_t)ncomp * K * K * K, s.parts, s.own, a.result);
    PS_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace psamd
