// pot_walk.hpp -- the potential's walk over one list of bodies, shared by potential.hip (every listed particle's phi)
// and probe.hip (phi at a caller's points): the terms, their order and their association are written once, here
// (device-inline only).  potential.hip's header comment holds the definition.
#pragma once

#include "pair_math.hpp"

namespace psamd {

constexpr int POT_CHAIN = 64;                            // fp32 additions in one chain, a multiple of the group's 8

// Eight bodies from jj on, their terms added to the chain `a` in list order.  TAIL: only the first `rem` of them are
// bodies of the list (the others are read -- inside the buffer, see pot_walk -- and dropped).  SELF: the list is the
// lane's own cell's, body 0 has sorted index gj0: the lane's own entry is dropped.  MASK: body i is one of the list only
// if bit i of `keep` (wave-uniform) is set -- the members of a far set among eight level cells (pot_far_block); the others
// are read and dropped.
template <bool SELF, bool TAIL, bool MASK = false>
__device__ __forceinline__ void pot_group(const PairCtx &ctx, const float *__restrict__ sx, const float *__restrict__ sy,
                                          const float *__restrict__ sz, const float *__restrict__ sw, int jj, int rem,
                                          int gj0, float eps2f, float &a, unsigned keep = 0xffu)
{
    constexpr int NQ = 8;
    v2f qx[NQ / 2], qy[NQ / 2], qz[NQ / 2], qw[NQ / 2];
    load_group<NQ>(sx, sy, sz, sw, jj, qx, qy, qz, qw);
    PairRows<NQ> r;
    pairs_dist<NQ, false>(ctx, qx, qy, qz, 0.f, r);
    const v2f eps = {eps2f, eps2f};
    v2f t[NQ / 2];
#pragma unroll
    for (int i = 0; i < NQ / 2; i++) {
        const v2f e = r.d[i] + eps;
        v2f s; s.x = __builtin_amdgcn_rsqf(e.x); s.y = __builtin_amdgcn_rsqf(e.y);
        t[i] = qw[i] * s;
    }
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        float ti = (i & 1) ? t[i >> 1].y : t[i >> 1].x;
        if (TAIL && i >= rem) ti = 0.f;
        if (MASK && !((keep >> i) & 1u)) ti = 0.f;
        if (SELF && gj0 + jj + i == ctx.gi) ti = 0.f;
        a += ti;
    }
}

// n bodies from four planes of a snapshot (wave-uniform pointers: scalar loads), their terms carried on in acc.
// padded: eight floats past the list's end can be read in every plane (the own snapshot: create.hip allocates it so;
// not the gathered one) -- the ragged tail is then one group with its surplus dropped instead of up to seven single
// bodies.  Both forms add the same terms in the same order.
template <bool SELF>
__device__ __forceinline__ void pot_walk(const PairCtx &ctx, const float *__restrict__ sx, const float *__restrict__ sy,
                                         const float *__restrict__ sz, const float *__restrict__ sw, int n, int gj0,
                                         float eps2f, bool padded, double &acc)
{
    for (int j0 = 0; j0 < n; j0 += POT_CHAIN) {
        const int m = min(POT_CHAIN, n - j0);
        float a = 0.f;
        int jj = 0;
        for (; jj + 8 <= m; jj += 8) pot_group<SELF, false>(ctx, sx, sy, sz, sw, j0 + jj, 8, gj0, eps2f, a);
        if (jj < m) {
            if (padded) pot_group<SELF, true>(ctx, sx, sy, sz, sw, j0 + jj, m - jj, gj0, eps2f, a);
            else {
                // (one body at a time: each term is pot_group's -- pairs_dist<NQ, false>'s unfused r.r, the same eps add, rsq and
                // multiply -- and must stay so, or a slab's all-pairs phi leaves the single context's bits;
                // tests/test_gpu_potential.py holds the two against each other on a world of two)
                for (; jj < m; jj++) {
                    const int j = j0 + jj;
                    const float rx = sx[j] - ctx.xi, ry = sy[j] - ctx.yi, rz = sz[j] - ctx.zi;
                    const float d2 = rx * rx + ry * ry + rz * rz;
                    float ti = sw[j] * __builtin_amdgcn_rsqf(d2 + eps2f);
                    if (SELF && gj0 + j == ctx.gi) ti = 0.f;
                    a += ti;
                }
            }
        }
        acc += (double)a;
    }
}

// where an all-pairs context finds the cells beyond the stencil: the own snapshot (world 1: cells by local == global index,
// lengths from consecutive starts, padded) or the all-gathered snapshot of all ranks with its index by global cell (the
// force pass and psamd_potential on world > 1; a probe reads the own snapshot always)
struct PotFar {
    const float *buf;
    const int *start, *n;
    unsigned long long plane;
    int padded;
};

inline PotFar pot_far_of(const DevParams &P, const DeviceState &d, bool gathered)
{
    if (gathered) return PotFar{reinterpret_cast<const float *>(d.allg_in), d.gstart, d.gn, (unsigned long long)P.allg_cap, 0};
    return PotFar{d.snap_soa, d.cell_start, nullptr, (unsigned long long)P.sorted_cap, 1};
}

// Far-field contexts (PSAMD_POTENTIAL_FAR, PSAMD_PROBE_FAR; far_walk.hpp says where the moments are and which are members).
// One block of 64 level cells (wave-uniform pointers to its moments: scalar loads): the members' terms -- pot_group's, on
// FAST_MATH contexts too -- are ONE fp32 chain in index order started at +0, its sum carried on in acc.  A group of eight
// without a member adds eight zeros and is skipped: a chain that starts at +0 never becomes -0.
__device__ __forceinline__ void pot_far_block(const PairCtx &ctx, const float *__restrict__ sx, const float *__restrict__ sy,
                                              const float *__restrict__ sz, const float *__restrict__ sw,
                                              unsigned long long take, float eps2f, double &acc)
{
    float a = 0.f;
    for (int g = 0; g < 64; g += 8) {
        const unsigned keep = (unsigned)(take >> g) & 0xffu;
        if (keep == 0u) continue;
        pot_group<false, false, true>(ctx, sx, sy, sz, sw, g, 8, 0, eps2f, a, keep);
    }
    acc += (double)a;
}

}  // namespace psamd
