// farfield.hip -- far-field gravity from one monopole per cell (PSAMD_FLAG_FAR_MONOPOLE) or from a pyramid of them
// (PSAMD_FLAG_FAR_PYRAMID); neither is in the reference
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
                                                      float *__restrict__ mom, int *__restrict__ mom_j, int mom_cap,
                                                      double *__restrict__ sums)      // (the pyramid keeps the fp64 sums; else null)
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
        if (sums) { sums[c] = S; sums[mom_cap + c] = Sx; sums[2 * (size_t)mom_cap + c] = Sy; sums[3 * (size_t)mom_cap + c] = Sz; }
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
    launch_far_moments(st, P, d);
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

// ------------------------------------------------------------------ a pyramid of monopoles (PSAMD_FLAG_FAR_PYRAMID, not in the reference)
// The far monopoles' cost grows with the number of cells: G^3 - 27 bodies a particle.  Here farther mass comes in coarser
// cells.  Level 0 is the cell grid with k_cell_moments' moments, a level-(l+1) cell sums the fp64 sums of its (at most 8)
// children in index order; cell i's set is, at the top level, every cell not adjacent to i >> L, and at every level below,
// every cell whose parent is adjacent to i's parent and which is not itself adjacent to i >> l: every cell of the box
// beyond the stencil is under exactly one member.  The walk keeps k_far_monopole's shape -- dense tasks, wave-uniform
// moments as scalar operands, a body that is not the lane's entered with mass 0 -- with (task, level) items: part p of the
// partial sums is level L - p, so that the parts' sum in part order is ((stencil + level L) + level L-1) + ... + level 0.
// Within a level: blocks of 64 cells in index order, a block one chain from +0, the chain sums added in block order to +0.
// A block or a group of 8 in which no lane of the wave has a body adds zeros only and is skipped: below the top level that
// is everything outside the box of the children of the neighbours of the wave's parents, a few blocks of the level.

// One thread per cell of level l >= 1: the fp64 sums of its children in ascending child index, each started at +0.
__global__ __launch_bounds__(256) void k_level_moments(const FarLevels lev, int l, float *__restrict__ mom, int *__restrict__ mom_j,
                                                       double *__restrict__ sums, int mom_cap)
{
    const int Gp = lev.G[l], Gc = lev.G[l - 1], k = blockIdx.x * 256 + threadIdx.x;
    if (k >= Gp * Gp * Gp) return;
    const int k3 = k / (Gp * Gp), rem = k - k3 * Gp * Gp, k1 = rem / Gp, k2 = rem - k1 * Gp;
    const size_t cap = (size_t)mom_cap;
    const double *cs = sums + lev.off[l - 1];
    double S = 0.0, Sx = 0.0, Sy = 0.0, Sz = 0.0;
    for (int c3 = 2 * k3; c3 <= min(2 * k3 + 1, Gc - 1); c3++)
        for (int c1 = 2 * k1; c1 <= min(2 * k1 + 1, Gc - 1); c1++)
            for (int c2 = 2 * k2; c2 <= min(2 * k2 + 1, Gc - 1); c2++) {
                const int ci = (c3 * Gc + c1) * Gc + c2;
                S += cs[ci]; Sx += cs[cap + ci]; Sy += cs[2 * cap + ci]; Sz += cs[3 * cap + ci];
            }
    const int o = lev.off[l] + k;
    const bool none = S == 0.0;
    sums[o] = S; sums[cap + o] = Sx; sums[2 * cap + o] = Sy; sums[3 * cap + o] = Sz;
    mom[o] = none ? 0.f : (float)(Sx / S);
    mom[cap + o] = none ? 0.f : (float)(Sy / S);
    mom[2 * cap + o] = none ? 0.f : (float)(Sz / S);
    mom[3 * cap + o] = none ? 0.f : (float)S;
    mom_j[o] = (k3 << 20) | (k1 << 10) | k2;
}

// The moments of the frame's snapshot, of the cells (far monopoles) or of every level (the pyramid, which keeps the fp64
// sums): the pair stage forms them here, and so do psamd_potential and psamd_probe in their far form, whose window opens
// before the pair stage has run -- the same kernels on the same snapshot, the same bits in the same buffers.
void launch_far_moments(hipStream_t st, const DevParams &P, const DeviceState &d)
{
    const bool pyramid = (P.flags & PSAMD_FLAG_FAR_PYRAMID) != 0;
    k_cell_moments<<<(P.num_cells + 3) / 4, 256, 0, st>>>(P, d.cell_start, d.snap_soa, d.cell_mom, d.cell_mom_j, d.mom_cap,
                                                          pyramid ? d.lev_sum : nullptr);
    if (!pyramid) return;
    const FarLevels &lev = d.lev;
    for (int l = 1; l < lev.n; l++)
        k_level_moments<<<(lev.G[l] * lev.G[l] * lev.G[l] + 255) / 256, 256, 0, st>>>(lev, l, d.cell_mom, d.cell_mom_j, d.lev_sum, d.mom_cap);
}

// (6 waves a SIMD, not k_far_monopole's 7: the second compare per body costs registers -- at 7 the compiler's report shows 68
// bytes of scratch a lane in the exact instance, at 6 it shows 8 (80 VGPRs); by that report, not by a timing)
constexpr int PYRAMID_WAVES = 6;

template <int MODE>
__global__ __launch_bounds__(256, PYRAMID_WAVES) void k_far_pyramid(DevParams P, const SnapSoa snap4, const int *__restrict__ act_start,
                                                                           const int *__restrict__ dense_gi, const int *__restrict__ dense_cell,
                                                                           const FarCells far, const FarLevels lev, const float *__restrict__ mom,
                                                                           const int *__restrict__ mom_j, int mom_cap)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n_act = act_start[comp_count(P)];
    const int ntask = min((n_act + 63) >> 6, (int)(far.part_plane >> 6));      // (the partial sums' room: never short, see create.hip)
    const int nitem = ntask * lev.n, nwg = (nitem + 3) >> 2;
    for (int b = blockIdx.x; b < nwg; b += gridDim.x) {
    // level-major: the top level's items first
    const int slot = __builtin_amdgcn_readfirstlane(xcd_contiguous(b, nwg) * 4 + wave);
    if (slot >= nitem) continue;
    const int part = slot / ntask, T = slot - part * ntask, l = lev.n - 1 - part;
    const bool top = part == 0;
    int Gl = 0, off = 0;
#pragma unroll
    for (int k = 0; k < FAR_MAX_LEVELS; k++) if (k == l) { Gl = lev.G[k]; off = lev.off[k]; }
    const int r = T * 64 + lane;
    const bool valid = r < n_act;
    const int rr = valid ? r : T * 64;                      // (a lane past the end rides along on the task's first particle; nothing of it is stored)
    const int gi = dense_gi[rr], c = dense_cell[rr];
    const float4 me = snap4[gi];
    const int GG = P.G * P.G;
    const int i3 = c / GG, irem = c - i3 * GG, i1 = irem / P.G, i2 = irem - i1 * P.G;      // (world == 1: local cell == global cell)
    const int a1 = i1 >> l, a2 = i2 >> l, a3 = i3 >> l;     // the lane's cell of this level, and its parent
    const int p1 = a1 >> 1, p2 = a2 >> 1, p3 = a3 >> 1;
    const PairCtx ctx = {me.x, me.y, me.z, 0.f, 0, gi, false};
    const float eps2f = (float)P.eps2;
    // The cells of the wave's particles lie in a box given by the lowest and the highest of them (k_far_monopole).  Shifted
    // by the level it bounds the lanes' level cells; the bodies any lane may have to mask or to take are, at the top level,
    // the neighbours of those, and below it the children of the neighbours of their parents.  Scalar arithmetic.
    int lo1 = 0, hi1 = P.G - 1, lo2 = 0, hi2 = P.G - 1, lo3, hi3;
    {
        const int c_hi = __builtin_amdgcn_readfirstlane(wave_max_i(c)), c_lo = __builtin_amdgcn_readfirstlane(-wave_max_i(-c));
        const int b3lo = c_lo / GG, b3hi = c_hi / GG;
        lo3 = b3lo; hi3 = b3hi;
        if (b3lo == b3hi) {
            const int ra = c_lo - b3lo * GG, rb = c_hi - b3hi * GG, b1lo = ra / P.G, b1hi = rb / P.G;
            lo1 = b1lo; hi1 = b1hi;
            if (b1lo == b1hi) { lo2 = ra - b1lo * P.G; hi2 = rb - b1hi * P.G; }
        }
        if (top) {
            lo1 = (lo1 >> l) - 1; lo2 = (lo2 >> l) - 1; lo3 = (lo3 >> l) - 1;
            hi1 = (hi1 >> l) + 1; hi2 = (hi2 >> l) + 1; hi3 = (hi3 >> l) + 1;
        } else {
            lo1 = 2 * ((lo1 >> (l + 1)) - 1); lo2 = 2 * ((lo2 >> (l + 1)) - 1); lo3 = 2 * ((lo3 >> (l + 1)) - 1);
            hi1 = 2 * ((hi1 >> (l + 1)) + 1) + 1; hi2 = 2 * ((hi2 >> (l + 1)) + 1) + 1; hi3 = 2 * ((hi3 >> (l + 1)) + 1) + 1;
        }
        lo1 = max(lo1, 0); lo2 = max(lo2, 0); lo3 = max(lo3, 0);
        hi1 = min(hi1, Gl - 1); hi2 = min(hi2, Gl - 1); hi3 = min(hi3, Gl - 1);
    }
    // the top level takes every block; a level below only those that hold a cell of the box: every cell of the box has
    // its index between the box's corners'
    const int blk_lo = top ? 0 : ((lo3 * Gl + lo1) * Gl + lo2) >> 6;
    const int blk_hi = top ? (Gl * Gl * Gl + 63) >> 6 : (((hi3 * Gl + hi1) * Gl + hi2) >> 6) + 1;
    float px = 0.f, py = 0.f, pz = 0.f;                     // the level's sum
    for (int blk = blk_lo; blk < blk_hi; blk++) {
        // lane = cell: which of the block's 64 cells hold mass at all, and which of those lie in the box
        const int base = off + blk * 64;
        const int jp = mom_j[base + lane];
        const bool nz = mom[3 * (size_t)mom_cap + base + lane] != 0.f;
        const int j3 = jp >> 20, j1 = (jp >> 10) & 1023, j2 = jp & 1023;
        const unsigned long long nearm = __ballot(nz && j3 >= lo3 && j3 <= hi3 && j1 >= lo1 && j1 <= hi1 && j2 >= lo2 && j2 <= hi2);
        const unsigned long long evalm = top ? __ballot(nz) : nearm;      // (below the top level no lane has a body outside the box)
        if (evalm == 0ull) continue;                        // (a chain of nothing is +0, and the level's sum never is -0)
        const float *sx = mom + base, *sy = sx + mom_cap, *sz = sy + mom_cap, *sw = sz + mom_cap;
        float ax = 0.f, ay = 0.f, az = 0.f;                 // the block's chain
        int flag = 0;
        for (int g = 0; g < 64; g += 8) {
            if (((evalm >> g) & 0xffull) == 0ull) continue; // (eight bodies of mass 0, or in no lane's set, add eight zeros)
            v2f qx[4], qy[4], qz[4], qw[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                qx[i] = v2f{sx[g + 2 * i], sx[g + 2 * i + 1]};
                qy[i] = v2f{sy[g + 2 * i], sy[g + 2 * i + 1]};
                qz[i] = v2f{sz[g + 2 * i], sz[g + 2 * i + 1]};
                qw[i] = v2f{sw[g + 2 * i], sw[g + 2 * i + 1]};
            }
            if (((nearm >> g) & 0xffull) != 0ull) {
                // some lane may have to leave one of these out: it is adjacent to the lane's cell of this level (a finer
                // level or the stencil has its mass), or -- below the top -- its parent is not adjacent to the lane's parent
                // (a coarser level has it)
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int j = __builtin_amdgcn_readlane(jp, g + k);
                    const int J3 = j >> 20, J1 = (j >> 10) & 1023, J2 = j & 1023;
                    const bool adj = abs(J3 - a3) <= 1 && abs(J1 - a1) <= 1 && abs(J2 - a2) <= 1;
                    const bool par = top || (abs((J3 >> 1) - p3) <= 1 && abs((J1 >> 1) - p1) <= 1 && abs((J2 >> 1) - p2) <= 1);
                    const bool hit = adj || !par;
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

// ((stencil chain + level L) + level L-1) + ... + level 0: k_allpairs_combine over the nparts parts that were written
__global__ void k_pyramid_combine(DevParams P, const int *__restrict__ act_start, const int *__restrict__ dense_gi,
                                  const int *__restrict__ dense_cell, const FarCells far, int nparts, const ForceBuf force4)
{
    const int n = min(act_start[comp_count(P)], (int)far.part_plane);
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const int gi = dense_gi[r], lc = dense_cell[r];
        float4 a = force4.get(P, lc, gi);                   // (flag 0, not a kid: it is on the active list)
        for (int p = 0; p < nparts; p++) {
            const float4 b = far.part_acc[(size_t)p * far.part_plane + (size_t)r];
            a.x += b.x; a.y += b.y; a.z += b.z;
        }
        force4.put(P, lc, gi, a);
    }
}

// What ran before is the stencil's chain, as for launch_far_monopole; now the moments of every level, the walk, the sum.
void launch_far_pyramid(hipStream_t st, const DevParams &P, const DeviceState &d, bool fast, int64_t live_bound)
{
    const FarLevels &lev = d.lev;
    launch_far_moments(st, P, d);
    FarCells far;
    far.part_acc = d.part_acc; far.part_plane = (unsigned long long)d.part_tasks * 64;
    const int64_t dense_bound = far_dense_bound(P, d, live_bound);
    launch_dense_order(st, P, d);
    const SnapSoa snap4{d.snap_soa, (size_t)P.sorted_cap};
    const unsigned far_wgs = (unsigned)((dense_bound * lev.n + 3) / 4);
    if (fast) k_far_pyramid<2><<<far_wgs, 256, 0, st>>>(P, snap4, d.act_start, d.dense_gi, d.dense_cell, far, lev, d.cell_mom, d.cell_mom_j, d.mom_cap);
    else k_far_pyramid<1><<<far_wgs, 256, 0, st>>>(P, snap4, d.act_start, d.dense_gi, d.dense_cell, far, lev, d.cell_mom, d.cell_mom_j, d.mom_cap);
    k_pyramid_combine<<<(unsigned)((dense_bound * 64 + 255) / 256), 256, 0, st>>>(P, d.act_start, d.dense_gi, d.dense_cell, far, lev.n, force_buf(d));
}

}  // namespace psamd
