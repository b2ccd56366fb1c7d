// pair_math.hpp -- the pair arithmetic every file of the pair stage shares (device-inline only): the short sqrt /
// reciprocal, one pair and NQ pairs in the exact, lean and fast forms, the exact collision rule, the count of a
// stencil's adults
#pragma once

#include "kernels_common.hpp"

namespace psamd {

// ------------------------------------------------------------------ pair kernel
// Correctly rounded fp32 sqrt and reciprocal without the range/denormal scaffolding
// the compiler wraps around them: valid for normal inputs well inside the exponent
// range (the host only selects them when eps2^3 .. (3 (2L)^2 + eps2)^3 lies in
// [2^-60, 2^60]).  Each is one hardware estimate (v_rsq_f32 / v_rcp_f32, 1 ulp) plus
// one residual correction, and each is checked against the compiler's correctly
// rounded form over EVERY float of [2^-62, 2^62] by psamd_selftest_math
// (tests/test_gpu_math.py): zero mismatches.
__device__ __forceinline__ float sqrt_rn_short(float a)
{
    const float r = __builtin_amdgcn_rsqf(a);
    const float g = a * r;                      // ~sqrt(a)
    const float h = 0.5f * r;                   // ~1 / (2 sqrt(a))
    const float d = __builtin_fmaf(-g, g, a);   // exact residual
    return __builtin_fmaf(d, h, g);
}

__device__ __forceinline__ float rcp_rn_newton(float q)
{
    const float x = __builtin_amdgcn_rcpf(q);
    const float e = __builtin_fmaf(-q, x, 1.0f);
    return __builtin_fmaf(e, x, x);
}

// RN(1 / RN(sqrt(a))): the reference's 1.0f / sqrtf(a), two roundings.
__device__ __forceinline__ float inv_sqrt_selected(float six)
{
    return rcp_rn_newton(sqrt_rn_short(six));
}

// One transcendental instead of two: the reciprocal's Newton step starts from the rsq estimate
// itself (r ~ 1/sqrt(a) ~ 1/s).  That is RN(1/s) for every float of the range EXCEPT where s has
// an all-ones mantissa (1/s lies a hair above a rounding tie and the step lands on the tie: 124
// inputs in [2^-62, 2^62]); there the residual e is exactly 2^-24, which is what `tie` reports so
// that the caller can redo the group with inv_sqrt_selected.  Checked for every float of the
// range by psamd_selftest_math: no mismatch that is not reported.  v_rcp_f32 costs 3.3 issue
// slots on gfx950 (profiles/r1_microbench_valu_rates.txt), the compare one.
__device__ __forceinline__ float inv_sqrt_guarded(float a, bool &tie)
{
    const float r = __builtin_amdgcn_rsqf(a);
    const float g = a * r, h = 0.5f * r;
    const float s = __builtin_fmaf(__builtin_fmaf(-g, g, a), h, g);
    const float e = __builtin_fmaf(-s, r, 1.0f);
    tie = tie || e == 0x1p-24f;
    return __builtin_fmaf(e, r, r);
}

// A tempting shortcut that is NOT exact, kept only so the self test can show it: start
// the reciprocal's Newton step from the rsq estimate (2h ~ 1/g) instead of a second
// transcendental.  124 of the 1.04e9 floats in range come out one ulp off.
__device__ __forceinline__ float inv_sqrt_one_transcendental(float a)
{
    const float r = __builtin_amdgcn_rsqf(a);
    float g = a * r, h = 0.5f * r;
    const float e = __builtin_fmaf(-h, g, 0.5f);
    h = __builtin_fmaf(h, e, h);
    g = __builtin_fmaf(g, e, g);
    const float q = __builtin_fmaf(__builtin_fmaf(-g, g, a), h, g);
    float x = h + h;
    for (int k = 0; k < 2; k++) x = __builtin_fmaf(__builtin_fmaf(-q, x, 1.0f), x, x);
    return x;
}

// bodyBodyInteraction, app_common.cu:236-267, for a snapshot body q = (x,y,z,w_eff).
__device__ __forceinline__ float pair_exact(float xi, float yi, float zi, const float4 q, double eps2,
                                            float &ax, float &ay, float &az)
{
    const float rx = q.x - xi, ry = q.y - yi, rz = q.z - zi;
    const float d2 = rx * rx + ry * ry + rz * rz;
    const float dsq = (float)((double)d2 + eps2);      // EPS2 is a double literal
    const float six = dsq * dsq * dsq;
    const float inv = 1.0f / sqrtf(six);               // correctly rounded sqrt, then divide
    const float s = q.w * inv;
    ax += rx * s; ay += ry * s; az += rz * s;
    return d2;
}

// Same physics with fused multiply-adds and the hardware reciprocal square root:
// differs from the reference in the last bits (PSAMD_FLAG_FAST_MATH).
__device__ __forceinline__ float pair_fast(float xi, float yi, float zi, const float4 q, float eps2,
                                           float &ax, float &ay, float &az)
{
    // One pair of pairsN_fast, operation for operation (the softened distance is ONE fma chain started at eps2): a body
    // gets the same bits whether it falls into a group of NQ or into the tail behind the groups, so the result does not
    // depend on NQ or on which walk the launch shape picked -- the same bytes from run to run and on any number of slabs.
    // Returns the softened squared distance, as pairsN_fast does.
    const float rx = q.x - xi, ry = q.y - yi, rz = q.z - zi;
    const float dsq = fmaf(rz, rz, fmaf(ry, ry, fmaf(rx, rx, eps2)));
    const float rinv = __builtin_amdgcn_rsqf(dsq);
    const float s = q.w * (rinv * rinv * rinv);
    ax = fmaf(rx, s, ax); ay = fmaf(ry, s, ay); az = fmaf(rz, s, az);
    return dsq;
}

// bodyBodyCollision, app_common.cu:269-301, evaluated exactly for the few pairs whose
// squared distance passes the gate.  0 none, 1 survive (higher id), 2 kill (lower id).
__device__ __forceinline__ int collide_exact(const DevParams &P, float d2, float age_i, int id_i,
                                             float age_j, int id_j)
{
    const float dist = sqrtf(d2);
    if ((double)dist > P.coll_radius || (double)age_i < P.kid_age || (double)age_j < P.kid_age) return 0;
    if ((double)age_i > P.life || (double)age_j > P.life) return 0;
    if (id_i > id_j) return 1;
    if (id_i < id_j) return 2;
    return 0;
}

// Lean exact pair arithmetic for k_pairs<1>.  The reference adds the double literal EPS2
// in double and rounds to float; from eps_f32_from upwards a plain fp32 add gives the same
// bits (checked for every such float when the context is created).  A wave takes the
// slow branch only when one of its lanes holds a pair closer than `slow_below` =
// max(eps_f32_from, collision gate): there EPS2 is added in double and the exact collision
// rule is evaluated for the pairs inside the gate, so the common path carries neither.
struct PairCtx {
    float xi, yi, zi, age_i;
    int id_i, gi;
    bool scan;
};

typedef float v2f __attribute__((ext_vector_type(2)));

// Two pairs per instruction slot: gfx950 has packed fp32 add/mul/fma, and the SoA tile hands
// (x_j, x_j+1) over in one aligned register pair, so nothing is shuffled between registers.
// Every packed operation rounds each half exactly like its scalar form.
__device__ __forceinline__ v2f inv_sqrt_selected2(v2f six)
{
    v2f r; r.x = __builtin_amdgcn_rsqf(six.x); r.y = __builtin_amdgcn_rsqf(six.y);
    const v2f g = six * r, h = 0.5f * r;
    const v2f s = __builtin_elementwise_fma(__builtin_elementwise_fma(-g, g, six), h, g);   // sqrt_rn_short
    v2f x; x.x = __builtin_amdgcn_rcpf(s.x); x.y = __builtin_amdgcn_rcpf(s.y);
    const v2f one = {1.0f, 1.0f};
    return __builtin_elementwise_fma(__builtin_elementwise_fma(-s, x, one), x, x);          // rcp_rn_newton
}

// inv_sqrt_guarded on two pairs
__device__ __forceinline__ v2f inv_sqrt_guarded2(v2f six, bool &tie)
{
    v2f r; r.x = __builtin_amdgcn_rsqf(six.x); r.y = __builtin_amdgcn_rsqf(six.y);
    const v2f g = six * r, h = 0.5f * r;
    const v2f s = __builtin_elementwise_fma(__builtin_elementwise_fma(-g, g, six), h, g);
    const v2f one = {1.0f, 1.0f};
    const v2f e = __builtin_elementwise_fma(-s, r, one);
    tie = tie || e.x == 0x1p-24f || e.y == 0x1p-24f;
    return __builtin_elementwise_fma(e, r, r);
}

// NQ pairs in two stages, so that a caller can start fetching the next group's bodies
// between them: distances first (the only use of the positions), then everything else.
template <int NQ>
struct PairRows {
    v2f rx[NQ / 2], ry[NQ / 2], rz[NQ / 2], d[NQ / 2];
    float dm;                                   // smallest d of the group
};

// SOFTENED: d = fma chain started at eps2 (fast math); else the reference's unfused r.r
template <int NQ, bool SOFTENED>
__device__ __forceinline__ void pairs_dist(const PairCtx &c, const v2f (&qx)[NQ / 2], const v2f (&qy)[NQ / 2],
                                           const v2f (&qz)[NQ / 2], float eps2, PairRows<NQ> &r)
{
    const v2f xi = {c.xi, c.xi}, yi = {c.yi, c.yi}, zi = {c.zi, c.zi}, eps = {eps2, eps2};
    r.dm = 3.0e38f;
#pragma unroll
    for (int i = 0; i < NQ / 2; i++) {
        r.rx[i] = qx[i] - xi; r.ry[i] = qy[i] - yi; r.rz[i] = qz[i] - zi;
        if (SOFTENED)
            r.d[i] = __builtin_elementwise_fma(r.rz[i], r.rz[i], __builtin_elementwise_fma(r.ry[i], r.ry[i], __builtin_elementwise_fma(r.rx[i], r.rx[i], eps)));
        else
            r.d[i] = r.rx[i] * r.rx[i] + r.ry[i] * r.ry[i] + r.rz[i] * r.rz[i];
        r.dm = fminf(fminf(r.dm, r.d[i].x), r.d[i].y);
    }
}

// ONE_T: one transcendental per pair (inv_sqrt_guarded2) -- fewer issue slots, for passes that are
// throughput-bound (four or more waves per SIMD: -3.7 % on the N = 2^20 force pass); the two-
// transcendental form has the shorter dependency chain and wins where a SIMD holds one or two waves
// (a 1/8 slab's tile walk: 0.57 against 0.64 ms).
// In two halves, so that a walk with a SIMD (almost) to itself can put the NEXT group's distances between them:
// pairs_scale_exact -- every pair's w / d^3 (the branches are in here) -- and pairs_add, the ordered additions.
template <int NQ, bool ONE_T>
__device__ __forceinline__ void pairs_scale_exact(const DevParams &P, const PairCtx &c, const PairRows<NQ> &r,
                                                  const v2f (&qw)[NQ / 2], int gj0,
                                                  const float *__restrict__ snap_age,
                                                  const int *__restrict__ sorted_id,
                                                  v2f (&sc)[NQ / 2], int &flag)
{
    constexpr int H = NQ / 2;
    v2f e[H];
    // One-pass stage (c.scan; a compile-time false in the two-pass force pass): a distance that is not a number --
    // the particle's own position or a body's is not one -- passes the reference's collision test, but the
    // group's minimum does not see it (fminf drops it): such a group takes the branch with the exact rule too.
    bool wild = false;
    if (c.scan) {
        v2f t = r.d[0];
#pragma unroll
        for (int i = 1; i < H; i++) t = t + r.d[i];
        const float tt = t.x + t.y;
        wild = tt != tt;
    }
    if (__any(r.dm < P.slow_below) || __any(wild)) {
#pragma unroll
        for (int i = 0; i < H; i++) {
            e[i].x = (float)((double)r.d[i].x + P.eps2);
            e[i].y = (float)((double)r.d[i].y + P.eps2);
        }
        if (c.scan && (wild || !(r.dm > P.coll_d2_gate))) {
#pragma unroll
            for (int i = 0; i < NQ; i++) {
                const float di = (i & 1) ? r.d[i >> 1].y : r.d[i >> 1].x;
                if (!(di > P.coll_d2_gate) && gj0 + i != c.gi)
                    flag = max(flag, collide_exact(P, di, c.age_i, c.id_i, snap_age[gj0 + i], sorted_id[gj0 + i]));
            }
        }
    } else {
        const v2f eps = {P.eps2f, P.eps2f};
#pragma unroll
        for (int i = 0; i < H; i++) e[i] = r.d[i] + eps;
    }
    if (!ONE_T) {
#pragma unroll
        for (int i = 0; i < H; i++) sc[i] = qw[i] * inv_sqrt_selected2(e[i] * e[i] * e[i]);
    } else {
        bool tie = false;
#pragma unroll
        for (int i = 0; i < H; i++) {
            sc[i] = inv_sqrt_guarded2(e[i] * e[i] * e[i], tie);
            // (keeps the step's last fma above the branch: sunk below it, its operands -- 16 VGPRs --
            // stay live across the branch and the kernel drops from 6 to 5 waves per SIMD)
            asm volatile("" : "+v"(sc[i]));
        }
        if (__any(tie)) {                               // about one group in 500
#pragma unroll
            for (int i = 0; i < H; i++) sc[i] = inv_sqrt_selected2(e[i] * e[i] * e[i]);
        }
#pragma unroll
        for (int i = 0; i < H; i++) sc[i] = qw[i] * sc[i];
    }
}

template <int NQ>
__device__ __forceinline__ void pairs_add(const PairRows<NQ> &r, const v2f (&sc)[NQ / 2], float &ax, float &ay, float &az)
{
#pragma unroll
    for (int i = 0; i < NQ / 2; i++) {                  // sums in list order
        const v2f px = r.rx[i] * sc[i], py = r.ry[i] * sc[i], pz = r.rz[i] * sc[i];
        ax += px.x; ay += py.x; az += pz.x;
        ax += px.y; ay += py.y; az += pz.y;
    }
}

template <int NQ, bool ONE_T>
__device__ __forceinline__ void pairs_finish_exact(const DevParams &P, const PairCtx &c, const PairRows<NQ> &r,
                                                   const v2f (&qw)[NQ / 2], int gj0,
                                                   const float *__restrict__ snap_age,
                                                   const int *__restrict__ sorted_id,
                                                   float &ax, float &ay, float &az, int &flag)
{
    v2f sc[NQ / 2];
    pairs_scale_exact<NQ, ONE_T>(P, c, r, qw, gj0, snap_age, sorted_id, sc, flag);
    pairs_add<NQ>(r, sc, ax, ay, az);
}

// Fast-math finish (FMA + v_rsq) on softened distances.
template <int NQ>
__device__ __forceinline__ void pairs_finish_fast(const PairRows<NQ> &r, const v2f (&qw)[NQ / 2],
                                                  float &ax, float &ay, float &az)
{
    constexpr int H = NQ / 2;
    v2f sc[H];
    // the group's transcendentals back to back: going from a transcendental to plain VALU work and back costs a
    // couple of cycles each way on gfx950 (profiles/r4_microbench_trans_overlap.txt: 8 v_rsq among 32 v_fma, one to
    // four, take 18 % longer than the same instructions grouped)
    v2f q[H];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < H; i++) { q[i].x = __builtin_amdgcn_rsqf(r.d[i].x); q[i].y = __builtin_amdgcn_rsqf(r.d[i].y); }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < H; i++) sc[i] = qw[i] * (q[i] * q[i] * q[i]);
#pragma unroll
    for (int i = 0; i < H; i++) {
        ax = fmaf(r.rx[i].x, sc[i].x, ax); ay = fmaf(r.ry[i].x, sc[i].x, ay); az = fmaf(r.rz[i].x, sc[i].x, az);
        ax = fmaf(r.rx[i].y, sc[i].y, ax); ay = fmaf(r.ry[i].y, sc[i].y, ay); az = fmaf(r.rz[i].y, sc[i].y, az);
    }
}

template <int NQ, bool ONE_T = true>
__device__ __forceinline__ void pairsN_exact_lean(const DevParams &P, const PairCtx &c, const v2f (&qx)[NQ / 2],
                                                  const v2f (&qy)[NQ / 2], const v2f (&qz)[NQ / 2],
                                                  const v2f (&qw)[NQ / 2], int gj0,
                                                  const float *__restrict__ snap_age,
                                                  const int *__restrict__ sorted_id,
                                                  float &ax, float &ay, float &az, int &flag)
{
    PairRows<NQ> r;
    pairs_dist<NQ, false>(c, qx, qy, qz, 0.f, r);
    pairs_finish_exact<NQ, ONE_T>(P, c, r, qw, gj0, snap_age, sorted_id, ax, ay, az, flag);
}

// returns the smallest softened squared distance (d2 + eps2) of the group, for the collision gate
template <int NQ>
__device__ __forceinline__ float pairsN_fast(const PairCtx &c, const v2f (&qx)[NQ / 2], const v2f (&qy)[NQ / 2],
                                             const v2f (&qz)[NQ / 2], const v2f (&qw)[NQ / 2], float eps2,
                                             float &ax, float &ay, float &az)
{
    PairRows<NQ> r;
    pairs_dist<NQ, true>(c, qx, qy, qz, eps2, r);
    pairs_finish_fast<NQ>(r, qw, ax, ay, az);
    return r.dm;
}

__device__ __forceinline__ void pair1_exact_lean(const DevParams &P, const PairCtx &c, const float4 q, int gj,
                                                 const float *__restrict__ snap_age,
                                                 const int *__restrict__ sorted_id,
                                                 float &ax, float &ay, float &az, int &flag)
{
    const float rx = q.x - c.xi, ry = q.y - c.yi, rz = q.z - c.zi;
    const float d2 = rx * rx + ry * ry + rz * rz;
    const float e = (float)((double)d2 + P.eps2);
    if (__any(c.scan && !(d2 > P.coll_d2_gate))) {
        if (c.scan && !(d2 > P.coll_d2_gate) && gj != c.gi)
            flag = max(flag, collide_exact(P, d2, c.age_i, c.id_i, snap_age[gj], sorted_id[gj]));
    }
    const float s = q.w * inv_sqrt_selected(e * e * e);
    ax += rx * s; ay += ry * s; az += rz * s;
}

// NQ bodies from jj on of four planes of a snapshot (wave-uniform pointers: scalar loads), two to a register pair
template <int NQ>
__device__ __forceinline__ void load_group(const float *sx, const float *sy, const float *sz, const float *sw, int jj, v2f (&qx)[NQ / 2], v2f (&qy)[NQ / 2],
                                           v2f (&qz)[NQ / 2], v2f (&qw)[NQ / 2])
{
#pragma unroll
    for (int i = 0; i < NQ / 2; i++) {
        qx[i] = v2f{sx[jj + 2 * i], sx[jj + 2 * i + 1]};
        qy[i] = v2f{sy[jj + 2 * i], sy[jj + 2 * i + 1]};
        qz[i] = v2f{sz[jj + 2 * i], sz[jj + 2 * i + 1]};
        qw[i] = v2f{sw[jj + 2 * i], sw[jj + 2 * i + 1]};
    }
}

// n bodies of one list (four planes, wave-uniform pointers) added to (ax, ay, az) in list order by the context's pair form:
// force.hip's walk_cell without its collision work -- the far cells of an all-pairs context (allpairs.hip), a probe's
// acceleration (probe.hip).  MATH 1: pairsN_exact_lean, and pair1_exact_lean for the ragged tail; 2: the fast forms;
// 0: pair_exact one body at a time, a massless body skipped as k_pairs<0> skips it.
template <int MATH, int NQ>
__device__ __forceinline__ void acc_walk(const DevParams &P, const PairCtx &ctx, const float *__restrict__ sx, const float *__restrict__ sy,
                                         const float *__restrict__ sz, const float *__restrict__ sw, int n, float eps2f,
                                         float &ax, float &ay, float &az)
{
    int flag = 0, jj = 0;
    if (MATH != 0) {
        for (; jj + NQ <= n; jj += NQ) {
            v2f qx[NQ / 2], qy[NQ / 2], qz[NQ / 2], qw[NQ / 2];
            // (load_group, spelled out: through the call k_allp_far<2, 8> comes out with other branches)
#pragma unroll
            for (int i = 0; i < NQ / 2; i++) {
                qx[i] = v2f{sx[jj + 2 * i], sx[jj + 2 * i + 1]};
                qy[i] = v2f{sy[jj + 2 * i], sy[jj + 2 * i + 1]};
                qz[i] = v2f{sz[jj + 2 * i], sz[jj + 2 * i + 1]};
                qw[i] = v2f{sw[jj + 2 * i], sw[jj + 2 * i + 1]};
            }
            if (MATH == 1) pairsN_exact_lean<NQ>(P, ctx, qx, qy, qz, qw, 0, nullptr, nullptr, ax, ay, az, flag);
            else (void)pairsN_fast<NQ>(ctx, qx, qy, qz, qw, eps2f, ax, ay, az);
        }
    }
    for (; jj < n; jj++) {
        const float4 q = make_float4(sx[jj], sy[jj], sz[jj], sw[jj]);
        if (MATH == 1) pair1_exact_lean(P, ctx, q, 0, nullptr, nullptr, ax, ay, az, flag);
        else if (MATH == 2) (void)pair_fast(ctx.xi, ctx.yi, ctx.zi, q, eps2f, ax, ay, az);
        else if (q.w != 0.0f) (void)pair_exact(ctx.xi, ctx.yi, ctx.zi, q, P.eps2, ax, ay, az);
    }
}

// Bodies in the stencil of local cell (i1, i2, i3) that are no kids, counted by one wave.  For the particle
// whose own position is not a number: the lean force walks let a particle meet itself and the kids because
// r * 0 adds nothing -- not so when r is no number.  The reference skips both (ps.cpp:1258,
// app_common.cu:240-243): with no other body in the stencil the particle's sum is +0 (this count is 1:
// itself), with one it is no number either way.
__device__ __forceinline__ int stencil_adults(const DevParams &P, int i1, int i2, int i3, const int *__restrict__ cell_start,
                                              const float *__restrict__ snap_age)
{
    const int lane = threadIdx.x & 63;
    int total = 0;
    for (int k = 0; k < STENCIL; k++) {
        const int nc = __builtin_amdgcn_readfirstlane(local_cell(P, i3 + c_stencil[k][2], i1 + c_stencil[k][1], i2 + c_stencil[k][0]));
        if (nc < 0) continue;
        const int b = __builtin_amdgcn_readfirstlane(cell_start[nc]);
        const int n = __builtin_amdgcn_readfirstlane(min(cell_start[nc + 1] - b, P.max_per_cell));
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            total += __popcll(__ballot(j < n && !(snap_age[b + (j < n ? j : 0)] < P.kid_thr)));
        }
    }
    return total;
}

}  // namespace psamd
