// far_walk.hpp -- what every walk over a far-field context's moments shares (PSAMD_FLAG_FAR_MONOPOLE, PSAMD_FLAG_FAR_PYRAMID):
// where the moments are, a level's place and size, the cells of a level that concern a range of grid cells, and the force
// pass's chain over one block of 64 level cells, the quadrupole terms of a far body -- acceleration and potential, on one shared
// front -- (PSAMD_FLAG_FAR_QUADRUPOLE).  The force pass (farfield.hip, k_far_walk), psamd_potential's far forms (potential.hip,
// k_pot_pairs<2> and <3>) and psamd_probe's (probe.hip, k_probe_pairs<.., 2> and <.., 3>) are written on these; device-inline only.
//
// The flat method is a pyramid of one level: its set is the top level's rule at level 0.  Cell i's set is, at the top level
// L, every cell that holds mass and is not adjacent to i >> L, and at a level l below it every such cell whose parent is
// adjacent to i's parent and which is not itself adjacent to i >> l (psamd.h, "a pyramid of monopoles").
#pragma once

#include "pair_math.hpp"

namespace psamd {

// Where a far-field context finds the moments the pair stage's own kernels form (farfield.hip): four planes X, Y, Z, M of
// mom_cap and the packed coordinates (pack_cell), every level padded with zeros to whole blocks of 64.
// nparts: the partial sums the force pass deals a level's blocks to (16 flat, 1 pyramid) -- the probe's acceleration
// repeats them.  A level's size and place follow from nlev and G (far_level): a few scalar operations.
struct FarMoments {
    const float *mom;
    const int *mom_j;
    int mom_cap, nparts;
    int nlev, G;            // L + 1 and G_0
};

inline FarMoments far_moments_of(const DevParams &P, const DeviceState &d)
{
    return FarMoments{d.cell_mom, d.cell_mom_j, d.mom_cap, (P.flags & PSAMD_FLAG_FAR_PYRAMID) ? 1 : ALLP_PARTS, d.lev.n, P.G};
}

// Level l (wave-uniform): G_l cells an axis at off .. off + G_l^3 of the planes, nblk blocks of 64 (far_levels_of's rule).
struct FarLevel {
    int G, off, nblk;
    bool top;
};

__device__ __forceinline__ FarLevel far_level(const FarMoments &m, int l)
{
    FarLevel v;
    v.G = m.G; v.off = 0;
    for (int k = 0; k < l; k++) { v.off += (v.G * v.G * v.G + 63) / 64 * 64; v.G = (v.G + 1) / 2; }
    v.nblk = (v.G * v.G * v.G + 63) >> 6;
    v.top = l == m.nlev - 1;
    return v;
}

// A box of cells, of the grid or of a level: lo .. hi on each axis (1 ~ i1, 2 ~ i2, 3 ~ i3).
struct FarBox {
    int lo1, hi1, lo2, hi2, lo3, hi3;
};

// Particles whose grid cells lie in `cells`: the cells of level l any of them may have to leave out or to take -- at the top
// level the neighbours of their level cells, below it the children of the neighbours of their parents -- clamped to the level.
__device__ __forceinline__ FarBox far_box(const FarLevel &v, int l, const FarBox &cells)
{
    FarBox b;
    if (v.top) {
        b.lo1 = (cells.lo1 >> l) - 1; b.lo2 = (cells.lo2 >> l) - 1; b.lo3 = (cells.lo3 >> l) - 1;
        b.hi1 = (cells.hi1 >> l) + 1; b.hi2 = (cells.hi2 >> l) + 1; b.hi3 = (cells.hi3 >> l) + 1;
    } else {
        b.lo1 = 2 * ((cells.lo1 >> (l + 1)) - 1); b.lo2 = 2 * ((cells.lo2 >> (l + 1)) - 1); b.lo3 = 2 * ((cells.lo3 >> (l + 1)) - 1);
        b.hi1 = 2 * ((cells.hi1 >> (l + 1)) + 1) + 1; b.hi2 = 2 * ((cells.hi2 >> (l + 1)) + 1) + 1; b.hi3 = 2 * ((cells.hi3 >> (l + 1)) + 1) + 1;
    }
    b.lo1 = max(b.lo1, 0); b.lo2 = max(b.lo2, 0); b.lo3 = max(b.lo3, 0);
    b.hi1 = min(b.hi1, v.G - 1); b.hi2 = min(b.hi2, v.G - 1); b.hi3 = min(b.hi3, v.G - 1);
    return b;
}

// The blocks [blk_lo, blk_hi) of the level that can hold a member of a set: all of the top level, below it those with a
// cell of the box (every cell of the box has its index between the box's corners').
__device__ __forceinline__ void far_blocks(const FarLevel &v, const FarBox &b, int &blk_lo, int &blk_hi)
{
    blk_lo = v.top ? 0 : ((b.lo3 * v.G + b.lo1) * v.G + b.lo2) >> 6;
    blk_hi = v.top ? v.nblk : (((b.hi3 * v.G + b.hi1) * v.G + b.hi2) >> 6) + 1;
}

// must a particle whose cell of the level is (a1, a2, a3) leave out the level cell with packed coordinates j?  It is adjacent
// to the particle's own (a finer level or the stencil has its mass) or -- below the top -- its parent is not adjacent to the
// particle's parent (a coarser level has it).
__device__ __forceinline__ bool far_leaves_out(bool top, int j, int a1, int a2, int a3)
{
    const int J3 = packed_i3(j), J1 = packed_i1(j), J2 = packed_i2(j);
    const bool adj = abs(J3 - a3) <= 1 && abs(J1 - a1) <= 1 && abs(J2 - a2) <= 1;
    const bool par = top || (abs((J3 >> 1) - (a3 >> 1)) <= 1 && abs((J1 >> 1) - (a1 >> 1)) <= 1 && abs((J2 >> 1) - (a2 >> 1)) <= 1);
    return adj || !par;
}

// Level l as the ONE cell (i1, i2, i3) sees it (potential and probe: all lanes of a wave walk one cell's set): the level, the
// cell's cell of the level and the blocks that can hold a member.  Wave-uniform: scalar arithmetic.
struct FarLevelView {
    FarLevel lev;
    int a1, a2, a3, blk_lo, blk_hi;
};

__device__ __forceinline__ FarLevelView far_level_view(const FarMoments &m, int l, int i1, int i2, int i3)
{
    FarLevelView v;
    v.lev = far_level(m, l);
    v.a1 = i1 >> l; v.a2 = i2 >> l; v.a3 = i3 >> l;
    far_blocks(v.lev, far_box(v.lev, l, FarBox{i1, i1, i2, i2, i3, i3}), v.blk_lo, v.blk_hi);
    return v;
}

// lane = cell of block blk of the level: the members of the cell's set, as a wave-uniform mask.  A member holds mass (M != 0:
// a moment that is no number counts) and is not left out.
__device__ __forceinline__ unsigned long long far_members(const FarMoments &m, const FarLevelView &v, int blk, int lane)
{
    const int at = v.lev.off + blk * 64 + lane;
    const bool nz = m.mom[3 * (size_t)m.mom_cap + at] != 0.f;
    return __ballot(nz && !far_leaves_out(v.lev.top, m.mom_j[at], v.a1, v.a2, v.a3));
}

// One block of 64 level cells (wave-uniform pointers to its moments: scalar loads) as ONE fp32 chain per component from +0,
// in index order, through the context's pair form (MATH 1: pairsN_exact_lean, 2: pairsN_fast), eight cells to a call.  A
// group of eight with no bit in evalm holds nothing any lane evaluates -- eight zeros -- and is skipped; leave(g, qw) zeroes
// the masses of the group's cells that are not the lane's: such a body adds +-0 to a chain that started at +0, the same bits
// as skipping it.  This is the force pass's association; the probe's acceleration repeats it with a wave-uniform mask.
// after(g, qx, qy, qz, qw): what else a walk does with the group's eight bodies, behind their pair terms (the quadrupole chain)
template <int MATH, class Leave, class After>
__device__ __forceinline__ void far_block_chain(const DevParams &P, const PairCtx &ctx, const float *__restrict__ sx,
                                                const float *__restrict__ sy, const float *__restrict__ sz,
                                                const float *__restrict__ sw, unsigned long long evalm, float eps2f,
                                                Leave leave, After after, float &ax, float &ay, float &az)
{
    ax = 0.f; ay = 0.f; az = 0.f;
    int flag = 0;
    for (int g = 0; g < 64; g += 8) {
        if (((evalm >> g) & 0xffull) == 0ull) continue;
        v2f qx[4], qy[4], qz[4], qw[4];
        // (load_group, spelled out: through the call the fast instances of k_far_walk come out with other code)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            qx[i] = v2f{sx[g + 2 * i], sx[g + 2 * i + 1]};
            qy[i] = v2f{sy[g + 2 * i], sy[g + 2 * i + 1]};
            qz[i] = v2f{sz[g + 2 * i], sz[g + 2 * i + 1]};
            qw[i] = v2f{sw[g + 2 * i], sw[g + 2 * i + 1]};
        }
        leave(g, qw);
        if (MATH == 1) pairsN_exact_lean<8>(P, ctx, qx, qy, qz, qw, 0, nullptr, nullptr, ax, ay, az, flag);
        else (void)pairsN_fast<8>(ctx, qx, qy, qz, qw, eps2f, ax, ay, az);
        after(g, qx, qy, qz, qw);
    }
}

template <int MATH, class Leave>
__device__ __forceinline__ void far_block_chain(const DevParams &P, const PairCtx &ctx, const float *__restrict__ sx,
                                                const float *__restrict__ sy, const float *__restrict__ sz,
                                                const float *__restrict__ sw, unsigned long long evalm, float eps2f,
                                                Leave leave, float &ax, float &ay, float &az)
{
    far_block_chain<MATH>(P, ctx, sx, sy, sz, sw, evalm, eps2f, leave, [](int, v2f (&)[4], v2f (&)[4], v2f (&)[4], v2f (&)[4]) {}, ax, ay, az);
}

// body k of a group of eight out of the chain: its mass becomes 0
__device__ __forceinline__ void far_drop(v2f (&qw)[4], int k, bool drop)
{
    if (k & 1) qw[k >> 1].y = drop ? 0.f : qw[k >> 1].y; else qw[k >> 1].x = drop ? 0.f : qw[k >> 1].x;
}

// ---- quadrupoles on the pyramid (PSAMD_FLAG_FAR_QUADRUPOLE) ----
// ONE far body at (X, Y, Z) with the central second moments C = (Cxx, Cyy, Czz, Cxy, Cxz, Cyz) seen from (xi, yi, zi): what
// its quadrupole acceleration and its quadrupole potential share -- d = (X, Y, Z) - x, the powers of u = (d.d + eps2)^(-1/2),
// g = C d, q = d.C.d, T = Cxx + Cyy + Czz.  The ONE form of every context, exact and PSAMD_FLAG_FAST_MATH alike, and of every
// kernel that inlines it: each multiply-add is an explicit fmaf or explicitly unfused (__fmul_rn, __fadd_rn), so the bits do
// not depend on the compiler's contraction setting or on the code around the call.  The operation sequence is psamd.h's
// ("quadrupoles on the pyramid"), line for line.
struct FarQuadFront {
    float dx, dy, dz, u3, u5, u7, gx, gy, gz, q, T;      // (u7: the acceleration's alone -- dead code where only phi is formed)
};

__device__ __forceinline__ FarQuadFront far_quad_front(float xi, float yi, float zi, float X, float Y, float Z, float cxx,
                                                       float cyy, float czz, float cxy, float cxz, float cyz, float eps2f)
{
    FarQuadFront f;
    f.dx = X - xi; f.dy = Y - yi; f.dz = Z - zi;                        // as the pair forms form it
    const float r2 = __fadd_rn(__fadd_rn(__fmul_rn(f.dx, f.dx), __fmul_rn(f.dy, f.dy)), __fmul_rn(f.dz, f.dz));
    const float u = __builtin_amdgcn_rsqf(__fadd_rn(r2, eps2f));
    const float u2 = __fmul_rn(u, u);
    f.u3 = __fmul_rn(u2, u); f.u5 = __fmul_rn(f.u3, u2); f.u7 = __fmul_rn(f.u5, u2);
    f.gx = fmaf(cxz, f.dz, fmaf(cxy, f.dy, __fmul_rn(cxx, f.dx)));      // C d
    f.gy = fmaf(cyz, f.dz, fmaf(cyy, f.dy, __fmul_rn(cxy, f.dx)));
    f.gz = fmaf(czz, f.dz, fmaf(cyz, f.dy, __fmul_rn(cxz, f.dx)));
    f.q = fmaf(f.gz, f.dz, fmaf(f.gy, f.dy, __fmul_rn(f.gx, f.dx)));    // d.C.d
    f.T = __fadd_rn(__fadd_rn(cxx, cyy), czz);
    return f;
}

// The quadrupole acceleration, the second-order Taylor term of the softened kernel about the body's centre of mass:
//   a_q = -3 (C d) u^5 + 7.5 (d.C.d) u^7 d - 1.5 T u^5 d
__device__ __forceinline__ void far_quad_acc(const FarQuadFront &f, float &tx, float &ty, float &tz)
{
    const float s = fmaf(__fmul_rn(7.5f, f.u7), f.q, __fmul_rn(__fmul_rn(-1.5f, f.T), f.u5));      // what multiplies d
    const float m3 = __fmul_rn(-3.0f, f.u5);
    tx = fmaf(m3, f.gx, __fmul_rn(s, f.dx)); ty = fmaf(m3, f.gy, __fmul_rn(s, f.dy)); tz = fmaf(m3, f.gz, __fmul_rn(s, f.dz));
}

// The quadrupole potential in the convention of the potential's sums (sum of w u, phi = -sum): the term whose gradient is a_q,
//   t_q = 1.5 (d.C.d) u^5 - 0.5 T u^3
__device__ __forceinline__ float far_quad_phi(const FarQuadFront &f)
{
    return fmaf(__fmul_rn(1.5f, f.u5), f.q, __fmul_rn(__fmul_rn(-0.5f, f.T), f.u3));
}

__device__ __forceinline__ void far_quad_term(float xi, float yi, float zi, float X, float Y, float Z, float cxx, float cyy,
                                              float czz, float cxy, float cxz, float cyz, float eps2f, float &tx, float &ty,
                                              float &tz)
{
    far_quad_acc(far_quad_front(xi, yi, zi, X, Y, Z, cxx, cyy, czz, cxy, cxz, cyz, eps2f), tx, ty, tz);
}

// The quadrupole terms of a group of eight level cells, added in index order to the block's quadrupole chains: (bx, by, bz)
// of the acceleration (ACC) and bp of the potential (PHI); a body's front is formed once for both.
// c6: the block's Cxx plane at the group (wave-uniform: scalar loads), the five other planes mom_cap apart.  qw: the group's
// masses AFTER the lane's leave-outs -- a body whose mass is 0 there is no member of the lane's set: +0 is added in its
// place, which leaves every bit of the chain as it is.
template <bool ACC, bool PHI>
__device__ __forceinline__ void far_quad_group(const PairCtx &ctx, const v2f (&qx)[4], const v2f (&qy)[4], const v2f (&qz)[4],
                                               const v2f (&qw)[4], const float *__restrict__ c6, int mom_cap, float eps2f,
                                               float &bx, float &by, float &bz, float &bp)
{
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const bool odd = (k & 1) != 0;
        const float X = odd ? qx[k >> 1].y : qx[k >> 1].x, Y = odd ? qy[k >> 1].y : qy[k >> 1].x, Z = odd ? qz[k >> 1].y : qz[k >> 1].x;
        const bool in = (odd ? qw[k >> 1].y : qw[k >> 1].x) != 0.f;
        const float *c = c6 + k;
        const FarQuadFront f = far_quad_front(ctx.xi, ctx.yi, ctx.zi, X, Y, Z, c[0], c[mom_cap], c[2 * (size_t)mom_cap],
                                              c[3 * (size_t)mom_cap], c[4 * (size_t)mom_cap], c[5 * (size_t)mom_cap], eps2f);
        if (ACC) {
            float tx, ty, tz;
            far_quad_acc(f, tx, ty, tz);
            bx = __fadd_rn(bx, in ? tx : 0.f); by = __fadd_rn(by, in ? ty : 0.f); bz = __fadd_rn(bz, in ? tz : 0.f);
        }
        if (PHI) bp = __fadd_rn(bp, in ? far_quad_phi(f) : 0.f);
    }
}

// (the force pass's: the acceleration alone)
__device__ __forceinline__ void far_quad_group(const PairCtx &ctx, const v2f (&qx)[4], const v2f (&qy)[4], const v2f (&qz)[4],
                                               const v2f (&qw)[4], const float *__restrict__ c6, int mom_cap, float eps2f,
                                               float &bx, float &by, float &bz)
{
    float none = 0.f;
    far_quad_group<true, false>(ctx, qx, qy, qz, qw, c6, mom_cap, eps2f, bx, by, bz, none);
}

// The quadrupole chain of the potential for one block of 64 level cells (wave-uniform pointers to its X, Y, Z planes and its
// Cxx plane: scalar loads), behind the block's monopole chain (pot_walk.hpp, pot_far_block): ONE fp32 chain from +0, in index
// order, over the members `take` (wave-uniform) of the monopole chain, its sum carried on in acc by an addition of its own.
// A group of eight without a member adds eight zeros and is skipped.
__device__ __forceinline__ void far_quad_phi_block(const PairCtx &ctx, const float *__restrict__ sx, const float *__restrict__ sy,
                                                   const float *__restrict__ sz, const float *__restrict__ sc, int mom_cap,
                                                   unsigned long long take, float eps2f, double &acc)
{
    float a = 0.f;
    for (int g = 0; g < 64; g += 8) {
        const unsigned keep = (unsigned)(take >> g) & 0xffu;
        if (keep == 0u) continue;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float *c = sc + g + k;
            const FarQuadFront f = far_quad_front(ctx.xi, ctx.yi, ctx.zi, sx[g + k], sy[g + k], sz[g + k], c[0], c[mom_cap],
                                                  c[2 * (size_t)mom_cap], c[3 * (size_t)mom_cap], c[4 * (size_t)mom_cap],
                                                  c[5 * (size_t)mom_cap], eps2f);
            a = __fadd_rn(a, ((keep >> k) & 1u) ? far_quad_phi(f) : 0.f);
        }
    }
    acc += (double)a;
}

}  // namespace psamd
