// farfield.hip -- far-field gravity from monopoles: one per cell of the box (PSAMD_FLAG_FAR_MONOPOLE, the flat method) or a
// pyramid of them (PSAMD_FLAG_FAR_PYRAMID); neither is in the reference.  The moments' kernels, ONE force walk for both
// methods (k_far_walk) and its launch.
//
// A particle's acceleration = the stencil's chain, exactly force.hip's cutoff pass (the reference's order), plus its far set
// (far_walk.hpp): flat, every other cell of the box as ONE body -- the cell's total w_eff at its centre of mass
// (k_cell_moments); as a pyramid, farther mass in coarser cells -- level 0 is the cell grid, a level-(l+1) cell sums the fp64
// sums of its (at most 8) children in index order, and every cell of the box beyond the stencil is under exactly one member
// of the set.  The flat method's cost grows with the number of cells, G^3 - 27 bodies a particle; the pyramid's with log G.
//
// The walk goes by allpairs.hip's dense tasks -- the particles that need a force, in cell order, 64 to a wave whatever their
// cells -- and (task, part) items, one wave each; part p of the partial sums is
//   flat      the p-th sixteenth of level 0's blocks of 64 cells (level 0 is the top level: the top level's rule),
//   pyramid   level L - p, of which a wave walks the blocks that hold a cell of its box,
// so that k_allpairs_combine's sum in part order is ((stencil + part 0) + part 1) + ..., the pyramid's top level first.
// Within a part: blocks in index order, a block ONE chain of at most 64 additions from +0 (far_block_chain), the chains'
// sums added in block order to +0.  All 64 lanes walk the same cells, so the moments are wave-uniform loads, 8 to a call of
// the context's pair form.  What differs from lane to lane is which cells a lane must leave out (far_leaves_out: the cutoff
// pass, a finer or a coarser level has their mass): there the lane enters the cell with mass 0, which adds +-0 to a chain
// that started at +0 -- the same bits as skipping it.  A wave's particles come from a short run of cells, so nearly every
// group of 8 cells lies outside the box around everything any lane leaves out (far_box) and is walked with no per-lane
// work at all; the test for that is scalar.  Below the top level nothing outside that box is in any lane's set: such blocks
// and groups add zeros only and are skipped.  The association depends on nothing but G and the global cell order.
#include "far_walk.hpp"

namespace psamd {

// a double from another lane (k wave-uniform)
__device__ __forceinline__ double lane_f64(double v, int k)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

// Quadrupole contexts (PSAMD_FLAG_FAR_QUADRUPOLE) carry six sums more per cell of every level, the raw second moments
// S_ab = sum RN(RN(w_eff x_a) x_b) in the plane order xx, yy, zz, xy, xz, yz (the inner product is exact in fp64, the outer
// one rounding; every operation explicitly unfused), and six float planes of central moments behind X, Y, Z, M:
// C_ab = (float)(S_ab - RN(RN(S_a / S) S_b)), a the first index of the plane's name.  QUAD is a compile-time parameter of
// the moments' kernels and of the walk: the instances without it are what they were, instruction for instruction.
constexpr int QUAD_A[6] = {0, 1, 2, 0, 0, 1}, QUAD_B[6] = {0, 1, 2, 1, 2, 2};      // plane -> (a, b), 0 ~ x

__device__ __forceinline__ float far_central(double Sab, double Sa, double Sb, double S)
{
    return (float)__dsub_rn(Sab, __dmul_rn(__ddiv_rn(Sa, S), Sb));
}

// One wave per cell of the box (world == 1: local cell == global cell; a far slab: OWN, below).  The cell's list is the first
// min(count, MAX_PARTICLES_PER_CELL) entries of the sorted snapshot; S, Sx, Sy, Sz are fp64 sums over it IN LIST ORDER
// (entry 0 first, one addition per entry: the lanes fetch 64 entries at a time and every lane adds them one by one).  A
// product of two fp32 values is exact in fp64, so nothing here depends on contraction.
//
// OWN (a far slab, world > 1: PSAMD_FLAG_FAR_SLAB): one wave per OWN cell -- region 0, whose local index is the cell's
// offset in the rank's block of the all-gathered message -- and only the sums are kept: `sums` is the block's payload, its
// planes mom_cap = allg_cells doubles apart, `hdr` the block's header, which the first wave fills in.  The same loads, the
// same products, the same additions in the same order as on one context: the same sums.  The float planes and mom_j of the
// whole box are formed from the gathered sums (k_far_scatter).  The instances without OWN are what they were.
template <bool QUAD, bool OWN>
__global__ __launch_bounds__(256) void k_cell_moments(DevParams P, const int *__restrict__ cell_start, const float *__restrict__ snap,
                                                      float *__restrict__ mom, int *__restrict__ mom_j, int mom_cap,
                                                      double *__restrict__ sums,      // (the pyramid keeps the fp64 sums; else null)
                                                      int *__restrict__ hdr, const FrameScalars *__restrict__ fs)
{
    const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (OWN && c == 0 && lane == 0) { hdr[0] = P.n_own_cells; hdr[1] = QUAD ? 10 : 4; hdr[2] = fs->error; hdr[3] = P.reg_first[0] * P.G * P.G; }
    if (c >= (OWN ? P.n_own_cells : P.num_cells)) return;
    const int b = cell_start[c], n = min(cell_start[c + 1] - b, P.max_per_cell);
    const size_t cap = (size_t)P.sorted_cap;
    double S = 0.0, Sx = 0.0, Sy = 0.0, Sz = 0.0;
    double Q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        double w = 0.0, wx = 0.0, wy = 0.0, wz = 0.0;
        double q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (j < n) {
            w = (double)snap[3 * cap + b + j];
            wx = w * (double)snap[b + j]; wy = w * (double)snap[cap + b + j]; wz = w * (double)snap[2 * cap + b + j];
            if (QUAD) {
                const double wa[3] = {wx, wy, wz}, xb[3] = {(double)snap[b + j], (double)snap[cap + b + j], (double)snap[2 * cap + b + j]};
#pragma unroll
                for (int f = 0; f < 6; f++) q[f] = __dmul_rn(wa[QUAD_A[f]], xb[QUAD_B[f]]);
            }
        }
        const int m = min(64, n - j0);
        for (int k = 0; k < m; k++) {
            S += lane_f64(w, k); Sx += lane_f64(wx, k); Sy += lane_f64(wy, k); Sz += lane_f64(wz, k);
            if (QUAD) {
#pragma unroll
                for (int f = 0; f < 6; f++) Q[f] = __dadd_rn(Q[f], lane_f64(q[f], k));
            }
        }
    }
    if (OWN) {
        if (lane == 0) {
            sums[c] = S; sums[mom_cap + c] = Sx; sums[2 * (size_t)mom_cap + c] = Sy; sums[3 * (size_t)mom_cap + c] = Sz;
            if (QUAD) {
#pragma unroll
                for (int f = 0; f < 6; f++) sums[(4 + f) * (size_t)mom_cap + c] = Q[f];
            }
        }
        return;
    }
    if (lane == 0) {
        const bool none = S == 0.0;          // an empty cell, or kids only
        mom[c] = none ? 0.f : (float)(Sx / S);
        mom[mom_cap + c] = none ? 0.f : (float)(Sy / S);
        mom[2 * mom_cap + c] = none ? 0.f : (float)(Sz / S);
        mom[3 * mom_cap + c] = none ? 0.f : (float)S;
        int i1, i2, i3;
        global_coords(P, c, i1, i2, i3);
        mom_j[c] = pack_cell(i3, i1, i2);
        if (sums) { sums[c] = S; sums[mom_cap + c] = Sx; sums[2 * (size_t)mom_cap + c] = Sy; sums[3 * (size_t)mom_cap + c] = Sz; }
        if (QUAD) {
            const double Sa[3] = {Sx, Sy, Sz};
#pragma unroll
            for (int f = 0; f < 6; f++) {
                mom[(4 + f) * (size_t)mom_cap + c] = none ? 0.f : far_central(Q[f], Sa[QUAD_A[f]], Sa[QUAD_B[f]], S);
                sums[(4 + f) * (size_t)mom_cap + c] = Q[f];
            }
        }
    }
}

__device__ __forceinline__ int wave_max_i(int v)
{
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

// One thread per cell of level l >= 1: the fp64 sums of its children in ascending child index, each started at +0.
template <bool QUAD>
__global__ __launch_bounds__(256) void k_level_moments(const FarLevels lev, int l, float *__restrict__ mom, int *__restrict__ mom_j,
                                                       double *__restrict__ sums, int mom_cap)
{
    const int Gp = lev.G[l], Gc = lev.G[l - 1], k = blockIdx.x * 256 + threadIdx.x;
    if (k >= Gp * Gp * Gp) return;
    const int k3 = k / (Gp * Gp), rem = k - k3 * Gp * Gp, k1 = rem / Gp, k2 = rem - k1 * Gp;
    const size_t cap = (size_t)mom_cap;
    const double *cs = sums + lev.off[l - 1];
    double S = 0.0, Sx = 0.0, Sy = 0.0, Sz = 0.0;
    double Q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c3 = 2 * k3; c3 <= min(2 * k3 + 1, Gc - 1); c3++)
        for (int c1 = 2 * k1; c1 <= min(2 * k1 + 1, Gc - 1); c1++)
            for (int c2 = 2 * k2; c2 <= min(2 * k2 + 1, Gc - 1); c2++) {
                const int ci = (c3 * Gc + c1) * Gc + c2;
                S += cs[ci]; Sx += cs[cap + ci]; Sy += cs[2 * cap + ci]; Sz += cs[3 * cap + ci];
                if (QUAD) {
#pragma unroll
                    for (int f = 0; f < 6; f++) Q[f] = __dadd_rn(Q[f], cs[(4 + f) * cap + ci]);
                }
            }
    const int o = lev.off[l] + k;
    const bool none = S == 0.0;
    sums[o] = S; sums[cap + o] = Sx; sums[2 * cap + o] = Sy; sums[3 * cap + o] = Sz;
    mom[o] = none ? 0.f : (float)(Sx / S);
    mom[cap + o] = none ? 0.f : (float)(Sy / S);
    mom[2 * cap + o] = none ? 0.f : (float)(Sz / S);
    mom[3 * cap + o] = none ? 0.f : (float)S;
    mom_j[o] = pack_cell(k3, k1, k2);
    if (QUAD) {
        const double Sa[3] = {Sx, Sy, Sz};
#pragma unroll
        for (int f = 0; f < 6; f++) {
            sums[(4 + f) * cap + o] = Q[f];
            mom[(4 + f) * cap + o] = none ? 0.f : far_central(Q[f], Sa[QUAD_A[f]], Sa[QUAD_B[f]], S);
        }
    }
}

// levels 1..L of the pyramid from level 0's sums
static void launch_upper_levels(hipStream_t st, const DevParams &P, const DeviceState &d)
{
    const bool quad = (P.flags & PSAMD_FLAG_FAR_QUADRUPOLE) != 0;
    const FarLevels &lev = d.lev;
    for (int l = 1; l < lev.n; l++) {
        const unsigned wgs = (unsigned)((lev.G[l] * lev.G[l] * lev.G[l] + 255) / 256);
        const auto launch = [&](auto kernel) { kernel<<<wgs, 256, 0, st>>>(lev, l, d.cell_mom, d.cell_mom_j, d.lev_sum, d.mom_cap); };
        if (quad) launch(k_level_moments<true>); else launch(k_level_moments<false>);
    }
}

// The moments of the frame's snapshot, of the cells (far monopoles) or of every level (the pyramid, which keeps the fp64
// sums): the pair stage forms them here, and so do psamd_potential and psamd_probe in their far form, whose window opens
// before the pair stage has run -- the same kernels on the same snapshot, the same bits in the same buffers.
void launch_far_moments(hipStream_t st, const DevParams &P, const DeviceState &d)
{
    const bool pyramid = (P.flags & PSAMD_FLAG_FAR_PYRAMID) != 0, quad = (P.flags & PSAMD_FLAG_FAR_QUADRUPOLE) != 0;
    const unsigned cell_wgs = (unsigned)((P.num_cells + 3) / 4);
    const auto launch = [&](auto kernel) {      // (the pyramid keeps the fp64 sums: a quadrupole context is one)
        kernel<<<cell_wgs, 256, 0, st>>>(P, d.cell_start, d.snap_soa, d.cell_mom, d.cell_mom_j, d.mom_cap, pyramid ? d.lev_sum : nullptr, nullptr, nullptr);
    };
    if (quad) launch(k_cell_moments<true, false>); else launch(k_cell_moments<false, false>);
    if (pyramid) launch_upper_levels(st, P, d);
}

// ---- far field on slabs (PSAMD_FLAG_FAR_SLAB, world > 1) ----
// The moments of a cell depend on the cell's own list alone, and a level's on the level below: so every rank forms the fp64
// sums of its OWN cells (k_cell_moments<., true>, in slab_build, straight into allg_out), the hosts all-gather the blocks --
// 16 header words ([0] own cells, [1] planes, 4 or 10, [2] the sender's error bits, [3] its first global cell), then the
// planes S, Sx, Sy, Sz (and Sxx, Syy, Szz, Sxy, Sxz, Syz), allg_cells doubles each -- and every rank scatters all blocks to
// level 0 of lev_sum by global cell (k_far_scatter, in slab_pairs), forms level 0's float planes and mom_j from the sums by
// k_cell_moments' own operations, and adds up the levels above with k_level_moments as one context does: redundantly on
// every rank, O(cells).  Afterwards every rank holds the moment arrays of one context, bit for bit.
// By a kernel trace (profiles/far_slab_cost.txt: N = 2^20 on 16^3 cells, eight slabs one at a time on one MI355X; a rank and
// step, pyramid / quadrupoles): k_cell_moments<., OWN> 20-21 / 34-38 us for the two or three own layers (the whole box on
// one context: 54 / 116 us), k_far_scatter 5-6.5 / 5-8 us, the two upper levels together 9-10 / 11 us, as on one context:
// latency of small kernels, about 2 % of the rank's pair stage.
hipError_t launch_far_own_sums(hipStream_t st, const DevParams &P, const DeviceState &d, int *msg)
{
    const unsigned wgs = (unsigned)((std::max(P.n_own_cells, 1) + 3) / 4);
    double *pay = reinterpret_cast<double *>(msg + MSG_HEADER_WORDS);
    const auto launch = [&](auto kernel) { kernel<<<wgs, 256, 0, st>>>(P, d.cell_start, d.snap_soa, nullptr, nullptr, P.allg_cells, pay, msg, d.fs); };
    if (P.flags & PSAMD_FLAG_FAR_QUADRUPOLE) launch(k_cell_moments<true, true>); else launch(k_cell_moments<false, true>);
    return hipGetLastError();
}

// One thread per (gathered block, cell of it).  A block is taken only if its header says what the plan says of its rank
// (far_plan: first global cell, cells; the planes of this context) -- and the plan's numbers, not the header's, bound every
// index: a block that did not arrive, or another context's, raises ERR_SLAB_MISMATCH and is left out, it is never followed.
// (A well-formed block of the step before is not told from this step's.)  The senders' error bits are adopted as
// k_allg_index adopts them.
template <bool QUAD>
__global__ __launch_bounds__(256) void k_far_scatter(DevParams P, const int *__restrict__ all, const int *__restrict__ far_plan,
                                                     float *__restrict__ mom, int *__restrict__ mom_j, double *__restrict__ sums,
                                                     int mom_cap, FrameScalars *fs)
{
    const int r = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const int *hdr = all + (size_t)r * P.allg_block;
    const int first = far_plan[2 * r], ncell = far_plan[2 * r + 1];
    const bool plan_ok = first >= 0 && ncell >= 0 && ncell <= P.allg_cells && first + ncell <= P.num_cells_global && first + ncell <= mom_cap;
    if (!plan_ok || hdr[0] != ncell || hdr[3] != first || hdr[1] != (QUAD ? 10 : 4)) {
        if (j == 0) atomicOr(&fs->error, ERR_SLAB_MISMATCH);
        return;
    }
    if (j == 0 && hdr[2]) atomicOr(&fs->error, hdr[2]);
    if (j >= ncell) return;
    const double *pay = reinterpret_cast<const double *>(hdr + MSG_HEADER_WORDS);
    const size_t pc = (size_t)P.allg_cells, cap = (size_t)mom_cap;
    const int c = first + j;
    const double S = pay[j], Sx = pay[pc + j], Sy = pay[2 * pc + j], Sz = pay[3 * pc + j];
    const bool none = S == 0.0;
    sums[c] = S; sums[cap + c] = Sx; sums[2 * cap + c] = Sy; sums[3 * cap + c] = Sz;
    mom[c] = none ? 0.f : (float)(Sx / S);
    mom[cap + c] = none ? 0.f : (float)(Sy / S);
    mom[2 * cap + c] = none ? 0.f : (float)(Sz / S);
    mom[3 * cap + c] = none ? 0.f : (float)S;
    int i1, i2, i3;
    global_coords(P, c, i1, i2, i3);
    mom_j[c] = pack_cell(i3, i1, i2);
    if (QUAD) {
        const double Sa[3] = {Sx, Sy, Sz};
#pragma unroll
        for (int f = 0; f < 6; f++) {
            const double q = pay[(4 + f) * pc + j];
            sums[(4 + f) * cap + c] = q;
            mom[(4 + f) * cap + c] = none ? 0.f : far_central(q, Sa[QUAD_A[f]], Sa[QUAD_B[f]], S);
        }
    }
}

hipError_t launch_far_gathered(hipStream_t st, const DevParams &P, const DeviceState &d)
{
    const dim3 grid((unsigned)((std::max(P.allg_cells, 1) + 255) / 256), (unsigned)P.world);
    const auto launch = [&](auto kernel) { kernel<<<grid, 256, 0, st>>>(P, d.allg_in, d.far_plan, d.cell_mom, d.cell_mom_j, d.lev_sum, d.mom_cap, d.fs); };
    if (P.flags & PSAMD_FLAG_FAR_QUADRUPOLE) launch(k_far_scatter<true>); else launch(k_far_scatter<false>);
    if (P.flags & PSAMD_FLAG_FAR_PYRAMID) launch_upper_levels(st, P, d);
    return hipGetLastError();
}


// (the pyramid's instances at 6 waves a SIMD, not the flat ones' 7: the parent compare per body costs registers -- at 7 the
// compiler's report shows 68 bytes of scratch a lane in the exact instance, at 6 it shows 8 (80 VGPRs); by that report, not
// by a timing)
constexpr int PYRAMID_WAVES = 6;
// (the quadrupole instances at 5: by the compiler's report, at 6 they spill 48 (fast) and 104 (exact) bytes of scratch a lane
// in 80 VGPRs; at 5 the fast one takes 93 VGPRs and none, the exact one 96 and 8; at 4 the exact one takes 103 and none, which
// does not pay for a wave)
constexpr int QUAD_WAVES = 5;

// The force walk of both methods.  PYRAMID is a compile-time parameter: the flat instances have l = 0 and top = true as
// constants and carry neither the level arithmetic nor the parent compare.  mom, mom_j: at.mom and at.mom_j once more, as
// __restrict__ kernel arguments -- what tells the compiler that the store of the partial sums does not touch the moments, so
// that they stay scalar loads (a pointer inside a struct cannot say it).
//
// QUAD (PSAMD_FLAG_FAR_QUADRUPOLE, the pyramid only): every member adds its quadrupole term (far_walk.hpp, far_quad_term)
// to a chain of its own per block -- from +0, in index order, behind the group's pair terms -- whose sums add up in block
// order to +0 like the monopoles'; the part is RN(monopole sum + quadrupole sum).  The six C planes lie behind the four of
// mom, so they come through the same __restrict__ argument as wave-uniform loads.
//
// SLAB (a far slab, world > 1): dense_cell holds LOCAL cells -- the lent-in layers first, which lie below the own layers in
// the box -- so the lane's coordinates come from the region tables (cell_coords) and the wave's box from the lowest and the
// highest GLOBAL cell among its lanes.  The moments are the whole box's on every rank (k_far_scatter), the far set depends on
// the particle's global cell alone: the same chains as on one context.  A compile-time parameter: the world == 1
// instances are what they were.  By the compiler's report (VGPRs / bytes of scratch a lane; fast, exact): the world == 1
// instances take 72/72, 72/28 (flat), 79/0, 80/0 (pyramid), 93/0, 96/8 (quadrupoles), as before the parameter existed; the
// slab instances 72/84, 72/28, 79/0, 80/0, 94/0, 96/8 -- the region walk costs the flat fast one 12 bytes of scratch and
// the quadrupole fast one a register, at the same waves a SIMD.
template <int MODE, bool PYRAMID, bool QUAD, bool SLAB>
__global__ __launch_bounds__(256, QUAD ? QUAD_WAVES : PYRAMID ? PYRAMID_WAVES : BALANCED_WAVES) void k_far_walk(DevParams P, const SnapSoa snap4,
                                                                                             const int *__restrict__ act_start,
                                                                                             const int *__restrict__ dense_gi,
                                                                                             const int *__restrict__ dense_cell,
                                                                                             const FarCells far, const FarMoments at,
                                                                                             const float *__restrict__ mom,
                                                                                             const int *__restrict__ mom_j)
{
    const FarMoments m = {mom, mom_j, at.mom_cap, at.nparts, at.nlev, P.G};      // (P.G is at.G: one scalar fewer alive across the walk)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n_act = act_start[comp_count(P)];
    const int ntask = min((n_act + 63) >> 6, (int)(far.part_plane >> 6));      // (the partial sums' room: never short, see create.hip)
    const int nitem = ntask * (PYRAMID ? m.nlev : ALLP_PARTS), nwg = (nitem + 3) >> 2;
    // (the launch is sized from the host's bound of the live count, the items from the device's own count, as in k_allp_far)
    for (int b = blockIdx.x; b < nwg; b += gridDim.x) {
    // part-major, as in k_allp_far: an XCD's run of items reads one share of the moments (the pyramid's top level comes first)
    const int slot = __builtin_amdgcn_readfirstlane(xcd_contiguous(b, nwg) * 4 + wave);
    if (slot >= nitem) continue;
    const int part = slot / ntask, T = slot - part * ntask;
    const int l = PYRAMID ? m.nlev - 1 - part : 0;
    FarLevel lev = far_level(m, l);
    if (!PYRAMID) lev.top = true;                           // (one level: a constant for the compiler)
    const bool top = lev.top;
    const int r = T * 64 + lane;
    const bool valid = r < n_act;
    const int rr = valid ? r : T * 64;                      // (a lane past the end rides along on the task's first particle; nothing of it is stored)
    const int gi = dense_gi[rr], c = dense_cell[rr];
    const float4 me = snap4[gi];
    const int GG = P.G * P.G;
    int i1, i2, i3, cg = c;                                 // (world == 1: local cell == global cell)
    if (SLAB) { cell_coords(P, c, i1, i2, i3); cg = (i3 * P.G + i1) * P.G + i2; }
    else global_coords(P, c, i1, i2, i3);
    const int a1 = i1 >> l, a2 = i2 >> l, a3 = i3 >> l;     // the lane's cell of this level
    const PairCtx ctx = {me.x, me.y, me.z, 0.f, 0, gi, false};
    const float eps2f = (float)P.eps2;
    // The cells of the wave's particles lie in a box given by the lowest and the highest of them: every cell whose index
    // lies between the two has its coordinates in it.  far_box makes of it the level cells any lane may have to leave out
    // or to take.  Scalar arithmetic.
    FarBox box = {0, P.G - 1, 0, P.G - 1, 0, 0};
    {
        const int c_hi = __builtin_amdgcn_readfirstlane(wave_max_i(cg)), c_lo = __builtin_amdgcn_readfirstlane(-wave_max_i(-cg));
        box.lo3 = c_lo / GG; box.hi3 = c_hi / GG;
        if (box.lo3 == box.hi3) {
            const int ra = c_lo - box.lo3 * GG, rb = c_hi - box.hi3 * GG;
            box.lo1 = ra / P.G; box.hi1 = rb / P.G;
            if (box.lo1 == box.hi1) { box.lo2 = ra - box.lo1 * P.G; box.hi2 = rb - box.hi1 * P.G; }
        }
        box = far_box(lev, l, box);
    }
    int blk_lo, blk_hi;
    if (PYRAMID) far_blocks(lev, box, blk_lo, blk_hi);
    else { blk_lo = lev.nblk * part / ALLP_PARTS; blk_hi = lev.nblk * (part + 1) / ALLP_PARTS; }
    float px = 0.f, py = 0.f, pz = 0.f;                     // the part's sum
    float ux = 0.f, uy = 0.f, uz = 0.f;                     // ... and its quadrupole sum
    for (int blk = blk_lo; blk < blk_hi; blk++) {
        // lane = cell: which of the block's 64 cells hold mass at all, and which of those lie in the box
        const int base = lev.off + blk * 64;
        const int jp = m.mom_j[base + lane];
        const bool nz = m.mom[3 * (size_t)m.mom_cap + base + lane] != 0.f;
        const int j3 = packed_i3(jp), j1 = packed_i1(jp), j2 = packed_i2(jp);
        const unsigned long long nearm = __ballot(nz && j3 >= box.lo3 && j3 <= box.hi3 && j1 >= box.lo1 && j1 <= box.hi1 && j2 >= box.lo2 && j2 <= box.hi2);
        const unsigned long long evalm = top ? __ballot(nz) : nearm;      // (below the top level no lane has a body outside the box)
        if (evalm == 0ull) continue;                        // (a chain of nothing is +0, and the part's sum never is -0)
        const float *sx = m.mom + base, *sy = sx + m.mom_cap, *sz = sy + m.mom_cap, *sw = sz + m.mom_cap;
        float ax, ay, az;                                   // the block's chain
        float bx = 0.f, by = 0.f, bz = 0.f;                 // the block's quadrupole chain
        const auto leave = [&](int g, v2f (&qw)[4]) {
            // outside the box no lane leaves anything out; inside it every lane asks for its own cell
            if (((nearm >> g) & 0xffull) == 0ull) return;
#pragma unroll
            for (int k = 0; k < 8; k++) far_drop(qw, k, far_leaves_out(top, __builtin_amdgcn_readlane(jp, g + k), a1, a2, a3));
        };
        if (QUAD) {
            const float *sc = sw + m.mom_cap;
            far_block_chain<MODE>(P, ctx, sx, sy, sz, sw, evalm, eps2f, leave, [&](int g, v2f (&qx)[4], v2f (&qy)[4], v2f (&qz)[4], v2f (&qw)[4]) {
                far_quad_group(ctx, qx, qy, qz, qw, sc + g, m.mom_cap, eps2f, bx, by, bz);
            }, ax, ay, az);
            ux = __fadd_rn(ux, bx); uy = __fadd_rn(uy, by); uz = __fadd_rn(uz, bz);
        } else far_block_chain<MODE>(P, ctx, sx, sy, sz, sw, evalm, eps2f, leave, ax, ay, az);
        px += ax; py += ay; pz += az;
    }
    if (QUAD) { px = __fadd_rn(px, ux); py = __fadd_rn(py, uy); pz = __fadd_rn(pz, uz); }
    if (valid) far.part_acc[(size_t)part * far.part_plane + (size_t)r] = make_float4(px, py, pz, 0.f);
    }
}

template <bool PYRAMID, bool QUAD, bool SLAB>
static void launch_far_walk_as(hipStream_t st, unsigned wgs, const DevParams &P, const DeviceState &d, bool fast, const FarCells &far)
{
    const SnapSoa snap4{d.snap_soa, (size_t)P.sorted_cap};
    const FarMoments m = far_moments_of(P, d);
    if (fast) k_far_walk<2, PYRAMID, QUAD, SLAB><<<wgs, 256, 0, st>>>(P, snap4, d.act_start, d.dense_gi, d.dense_cell, far, m, m.mom, m.mom_j);
    else k_far_walk<1, PYRAMID, QUAD, SLAB><<<wgs, 256, 0, st>>>(P, snap4, d.act_start, d.dense_gi, d.dense_cell, far, m, m.mom, m.mom_j);
}

// (a slab's instances where the context is one: world > 1)
template <bool PYRAMID, bool QUAD>
static void launch_far_walk(hipStream_t st, unsigned wgs, const DevParams &P, const DeviceState &d, bool fast, const FarCells &far)
{
    if (P.world > 1) launch_far_walk_as<PYRAMID, QUAD, true>(st, wgs, P, d, fast, far);
    else launch_far_walk_as<PYRAMID, QUAD, false>(st, wgs, P, d, fast, far);
}

// What ran before is the stencil's chain (the two-pass pair stage: contexts with either flag are created only with it, only
// with lean arithmetic); now the moments, the walk by (dense task, part) items, the parts' sum.  A far slab (world > 1) has
// its moments already: psamd_slab_pairs formed them from the gathered sums (launch_far_gathered) before the pair stage; its
// dense tasks go over every cell the rank computes, lent-in layers included (comp_count), and the parts' sum lands where
// the cutoff pass left the record -- a lent layer's records then travel home in force_out.
void launch_far_field(hipStream_t st, const DevParams &P, const DeviceState &d, bool fast, int64_t live_bound)
{
    const bool pyramid = (P.flags & PSAMD_FLAG_FAR_PYRAMID) != 0;
    const int parts = pyramid ? d.lev.n : ALLP_PARTS;
    if (P.world == 1) launch_far_moments(st, P, d);
    FarCells far;
    far.part_acc = d.part_acc; far.part_plane = (unsigned long long)d.part_tasks * 64;
    const int64_t dense_bound = far_dense_bound(P, d, live_bound);
    launch_dense_order(st, P, d);
    const unsigned far_wgs = (unsigned)((dense_bound * parts + 3) / 4);
    if (P.flags & PSAMD_FLAG_FAR_QUADRUPOLE) launch_far_walk<true, true>(st, far_wgs, P, d, fast, far);
    else if (pyramid) launch_far_walk<true, false>(st, far_wgs, P, d, fast, far);
    else launch_far_walk<false, false>(st, far_wgs, P, d, fast, far);
    launch_far_combine(st, P, d, far, parts, dense_bound);
}

}  // namespace psamd
