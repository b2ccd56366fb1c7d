// farfield.hip -- far-field gravity from one monopole per cell (PSAMD_FLAG_FAR_MONOPOLE, not in the reference)
#include "pair_math.hpp"

namespace psamd {

// ------------------------------------------------------------------ far monopoles (PSAMD_FLAG_FAR_MONOPOLE, not in the reference)
// A particle's acceleration = the stencil's chain, exactly force.hip's cutoff pass (the reference's order), plus every
// other cell of the box in GLOBAL index order as ONE body: the cell's total w_eff at its centre of mass (k_cell_moments).
// The pass goes by allpairs.hip's dense tasks -- the particles that need a force, in cell order, 64 to a wave whatever
// their cells -- and its 16 parts: a wave (dense task, part) walks the 64-cell blocks of its part; a block's monopoles
// are ONE chain of at most 64 additions started at +0, the chain's sum is added to the part's, k_allpairs_combine adds
// the parts to the stencil's chain in part order.  All 64 lanes walk the same cells, so the monopoles are wave-uniform
// loads, 8 to a call of the context's pair form.  What differs from lane to lane is the 27 cells a lane must leave out
// (the cutoff pass has their bodies one by one): there the lane enters the cell with mass 0, which adds +-0 to a chain
// that started at +0 -- the same bits as skipping it.  A wave's particles come from a short run of cells, so nearly every
// group of 8 cells lies outside the box around all their stencils and is walked with no per-lane work at all; the
// test for that is scalar.  The association depends on nothing but G and the global cell order.

// a double from another lane (k wave-uniform)
__device__ __forceinline__ double lane_f64(double v, int k)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

// One wave per cell of the box (world == 1: local cell == global cell).  The cell's list is the first
// min(count, MAX_PARTICLES_PER_CELL) entries of the sorted snapshot; S, Sx, Sy, Sz are fp64 sums over it IN LIST ORDER
// (entry 0 first, one addition per entry: the lanes fetch 64 entries at a time and every lane adds them one by one).  A
// product of two fp32 values is exact in fp64, so nothing here depends on contraction.
__global__ __launch_bounds__(256) void k_cell_moments(DevParams P, const int *__restrict__ cell_start, const float *__restrict__ snap,
                                                      float *__restrict__ mom, int *__restrict__ mom_j, int mom_cap)
{
    const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (c >= P.num_cells) return;
    const int b = cell_start[c], n = min(cell_start[c + 1] - b, P.max_per_cell);
    const size_t cap = (size_t)P.sorted_cap;
    double S = 0.0, Sx = 0.0, Sy = 0.0, Sz = 0.0;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        double w = 0.0, wx = 0.0, wy = 0.0, wz = 0.0;
        if (j < n) {
            w = (double)snap[3 * cap + b + j];
            wx = w * (double)snap[b + j]; wy = w * (double)snap[cap + b + j]; wz = w * (double)snap[2 * cap + b + j];
        }
        const int m = min(64, n - j0);
        for (int k = 0; k < m; k++) { S += lane_f64(w, k); Sx += lane_f64(wx, k); Sy += lane_f64(wy, k); Sz += lane_f64(wz, k); }
    }
    if (lane == 0) {
        const bool none = S == 0.0;          // an empty cell, or kids only
        mom[c] = none ? 0.f : (float)(Sx / S);
        mom[mom_cap + c] = none ? 0.f : (float)(Sy / S);
        mom[2 * mom_cap + c] = none ? 0.f : (float)(Sz / S);
        mom[3 * mom_cap + c] = none ? 0.f : (float)S;
        const int GG = P.G * P.G, i3 = c / GG, rem = c - i3 * GG, i1 = rem / P.G;
        mom_j[c] = (i3 << 20) | (i1 << 10) | (rem - i1 * P.G);
    }
}

__device__ __forceinline__ int wave_max_i(int v)
{
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

template <int MODE>
__global__ __launch_bounds__(256, BALANCED_WAVES) void k_far_monopole(DevParams P, const SnapSoa snap4, const int *__restrict__ act_start,
                                                                            const int *__restrict__ dense_gi, const int *__restrict__ dense_cell,
                                                                            const FarCells far, const float *__restrict__ mom,
                                                                            const int *__restrict__ mom_j, int mom_cap)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n_act = act_start[comp_count(P)];
    const int ntask = min((n_act + 63) >> 6, (int)(far.part_plane >> 6));      // (the partial sums' room: never short, see create.hip)
    const int nitem = ntask * ALLP_PARTS, nwg = (nitem + 3) >> 2;
    // (the launch is sized from the host's bound of the live count, the items from the device's own count, as in k_allp_far)
    for (int b = blockIdx.x; b < nwg; b += gridDim.x) {
    // part-major, as in k_allp_far: an XCD's run of items reads one eighth of the monopoles
    const int slot = __builtin_amdgcn_readfirstlane(xcd_contiguous(b, nwg) * 4 + wave);
    if (slot >= nitem) continue;
    const int part = slot / ntask, T = slot - part * ntask;
    const int r = T * 64 + lane;
    const bool valid = r < n_act;
    const int rr = valid ? r : T * 64;                      // (a lane past the end rides along on the task's first particle; nothing of it is stored)
    const int gi = dense_gi[rr], c = dense_cell[rr];
    const float4 me = snap4[gi];
    const int GG = P.G * P.G;
    const int i3 = c / GG, irem = c - i3 * GG, i1 = irem / P.G, i2 = irem - i1 * P.G;      // (world == 1: local cell == global cell)
    const PairCtx ctx = {me.x, me.y, me.z, 0.f, 0, gi, false};
    const float eps2f = (float)P.eps2;
    // The box around the stencils of the wave's particles, from the lowest and the highest of their cells: every cell
    // whose index lies between the two has its coordinates in it.  Scalar arithmetic.
    int lo1 = 0, hi1 = P.G - 1, lo2 = 0, hi2 = P.G - 1, lo3, hi3;
    {
        const int c_hi = __builtin_amdgcn_readfirstlane(wave_max_i(c)), c_lo = __builtin_amdgcn_readfirstlane(-wave_max_i(-c));
        const int a3 = c_lo / GG, b3 = c_hi / GG;
        lo3 = a3; hi3 = b3;
        if (a3 == b3) {
            const int ra = c_lo - a3 * GG, rb = c_hi - b3 * GG, a1 = ra / P.G, b1 = rb / P.G;
            lo1 = a1; hi1 = b1;
            if (a1 == b1) { lo2 = ra - a1 * P.G; hi2 = rb - b1 * P.G; }
        }
        lo1--; lo2--; lo3--; hi1++; hi2++; hi3++;
    }
    const int nblk = (P.num_cells_global + 63) >> 6;        // (mom_cap == nblk * 64: the planes are padded with zeros)
    const int blk_lo = nblk * part / ALLP_PARTS, blk_hi = nblk * (part + 1) / ALLP_PARTS;
    float px = 0.f, py = 0.f, pz = 0.f;                     // the part's sum
    for (int blk = blk_lo; blk < blk_hi; blk++) {
        // lane = cell: which of the block's 64 cells hold mass at all, and which of those lie in the box
        const int jp = mom_j[blk * 64 + lane];
        const bool nz = mom[3 * (size_t)mom_cap + blk * 64 + lane] != 0.f;
        const int j3 = jp >> 20, j1 = (jp >> 10) & 1023, j2 = jp & 1023;
        const unsigned long long nzm = __ballot(nz);
        const unsigned long long nearm = __ballot(nz && j3 >= lo3 && j3 <= hi3 && j1 >= lo1 && j1 <= hi1 && j2 >= lo2 && j2 <= hi2);
        if (nzm == 0ull) continue;                          // (a chain of nothing is +0, and the part's sum never is -0)
        const float *sx = mom + (size_t)blk * 64, *sy = sx + mom_cap, *sz = sy + mom_cap, *sw = sz + mom_cap;
        float ax = 0.f, ay = 0.f, az = 0.f;                 // the block's chain
        int flag = 0;
        for (int g = 0; g < 64; g += 8) {
            if (((nzm >> g) & 0xffull) == 0ull) continue;   // (eight cells of mass 0 add eight zeros)
            v2f qx[4], qy[4], qz[4], qw[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                qx[i] = v2f{sx[g + 2 * i], sx[g + 2 * i + 1]};
                qy[i] = v2f{sy[g + 2 * i], sy[g + 2 * i + 1]};
                qz[i] = v2f{sz[g + 2 * i], sz[g + 2 * i + 1]};
                qw[i] = v2f{sw[g + 2 * i], sw[g + 2 * i + 1]};
            }
            if (((nearm >> g) & 0xffull) != 0ull) {
                // some lane may have one of these cells in its own stencil: the cutoff pass has its bodies
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int j = __builtin_amdgcn_readlane(jp, g + k);
                    const bool hit = abs((j >> 20) - i3) <= 1 && abs(((j >> 10) & 1023) - i1) <= 1 && abs((j & 1023) - i2) <= 1;
                    if (k & 1) qw[k >> 1].y = hit ? 0.f : qw[k >> 1].y; else qw[k >> 1].x = hit ? 0.f : qw[k >> 1].x;
                }
            }
            if (MODE == 1) pairsN_exact_lean<8>(P, ctx, qx, qy, qz, qw, 0, nullptr, nullptr, ax, ay, az, flag);
            else (void)pairsN_fast<8>(ctx, qx, qy, qz, qw, eps2f, ax, ay, az);
        }
        px += ax; py += ay; pz += az;
    }
    if (valid) far.part_acc[(size_t)part * far.part_plane + (size_t)r] = make_float4(px, py, pz, 0.f);
    }
}

// What ran before is the stencil's chain (the two-pass pair stage: contexts with the flag are created only with it, only
// with lean arithmetic and only with world == 1); now the cells' moments, every cell beyond the stencil as one body, the sum.
void launch_far_monopole(hipStream_t st, const DevParams &P, const DeviceState &d, bool fast, int64_t live_bound)
{
    k_cell_moments<<<(P.num_cells + 3) / 4, 256, 0, st>>>(P, d.cell_start, d.snap_soa, d.cell_mom, d.cell_mom_j, d.mom_cap);
    FarCells far;
    far.part_acc = d.part_acc; far.part_plane = (unsigned long long)d.part_tasks * 64;
    const int64_t dense_bound = far_dense_bound(P, d, live_bound);
    launch_dense_order(st, P, d);
    const SnapSoa snap4{d.snap_soa, (size_t)P.sorted_cap};
    const unsigned far_wgs = (unsigned)((dense_bound * ALLP_PARTS + 3) / 4);
    if (fast) k_far_monopole<2><<<far_wgs, 256, 0, st>>>(P, snap4, d.act_start, d.dense_gi, d.dense_cell, far, d.cell_mom, d.cell_mom_j, d.mom_cap);
    else k_far_monopole<1><<<far_wgs, 256, 0, st>>>(P, snap4, d.act_start, d.dense_gi, d.dense_cell, far, d.cell_mom, d.cell_mom_j, d.mom_cap);
    launch_far_combine(st, P, d, far, dense_bound);
}

}  // namespace psamd
