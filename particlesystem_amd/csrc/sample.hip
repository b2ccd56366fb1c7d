// sample.hip -- psamd_sample: a caller's lattice field read back at points, or at the live particles themselves, cloud-in-cell.
//
// Not part of the step and not in the reference.  The exact adjoint of psamd_deposit (deposit.hip): the
// same lattice (DepLattice), the same axis rule and the same fp32 weights (DepAxis, lattice.hpp) -- the weight a body gives a
// voxel there is the weight that voxel's value has in the body's sample here (include/psamd.h, "a lattice field at the
// particles").  A point is no particle and the call reads no frame: the geometry, the caller's lattice and, by export order, the
// context's pos4 and cell.  Behind a memset of the three counters:
//   k_sample<VEC4>        the points form.  One lane per entry, grid-stride over n; the 16-byte pos4 load, locate_cell (outside:
//                         the quiet NaNs and outcome 1), three DepAxis.  The eight voxels are four (n3, n1) rows of two
//                         n2-neighbours that are adjacent in memory: a row is one 8-byte load (float) or two 16-byte loads
//                         back to back (float4), and all four rows are issued before the first term is formed.  A voxel with an
//                         axis weight of exactly 0 is not loaded -- its lanes are switched off around the load, it costs no
//                         memory access -- and adds no term: n0 + 1 == M is never touched.  The terms RN(W v) go into one fp64
//                         chain per component in (d3, d1, d2) order; out = RN(scale (float)sum).  The 4- or 16-byte store, the
//                         outcome, and the three counts by wave ballot: one integer atomic per wave and count at the end.
//   k_sample_order<VEC4>  by export order, behind psamd_update's tile live-count pass (launch_live_tiles): workgroup t walks tile
//                         t of the owned slots, a live slot's entry k from tiles_before, wave_offset and lane_rank
//                         (slot_walk.hpp) as in k_update_order; SAMPLE_BATCH slots per lane have their cell words, then their
//                         positions, in flight together, and each goes through the same body.  (The tile's ballots are formed
//                         twice -- for the wave's count, then batch by batch -- so that no array of them is indexed by a loop
//                         counter; the second read of the cell words hits the cache.)
//   k_sample_finish       one thread: done = served + outside, the context's own record and the caller's.
// An entry's words depend on its position, the lattice and scale alone; no floating-point atomic anywhere.
//
// VGPRs / waves per SIMD as the compiler reports them for gfx950, no instance with scratch, no LDS beyond slot_walk.hpp's:
//   k_sample<float> 31 / 8    k_sample<float4> 59 / 8    k_sample_order<float> 48 / 8    k_sample_order<float4> 71 / 7
//   k_sample_finish 6 / 8
// (a gather: eight independent loads per entry and little arithmetic beside locate_cell's three fp64 divisions, so resident
// waves are what hides the latency; the float4 form by export order keeps a batch's positions beside a body's 32 loaded words)
// Measured at N = 2^20 (profiles/sample_cost.txt): 0.068-0.075 ms by export order, 0.090-0.092 ms for as many points.
#include "lattice.hpp"
#include "multisplit.hpp"

namespace psamd {

constexpr int SAMPLE_THREADS = 256;
constexpr int SAMPLE_MAX_BLOCKS = 2048;     // the points form's grid-stride launch: eight workgroups a CU
constexpr int SAMPLE_BATCH = 4;             // by export order: slots per lane whose cell words and positions are in flight together
enum { SH_SERVED = 0, SH_OUTSIDE, SH_NONFINITE };       // the header words (SAMPLE_HDR_WORDS); the first two are the outcome codes
static_assert(SH_NONFINITE < SAMPLE_HDR_WORDS && SLOT_ITEMS % SAMPLE_BATCH == 0, "a counter per count, whole batches per wave");

// a row's two n2-neighbours as one access (a float lattice is 4-byte aligned: the row need not start on 8 bytes)
struct __attribute__((packed, aligned(4))) SamplePair { float lo, hi; };

// Entry k at (x, y, z): its words into out[k], its outcome returned; nonfinite: a served entry with a word that is not finite
template <bool VEC4>
__device__ __forceinline__ int sample_entry(const DevParams &P, const SampleArgs &a, float x, float y, float z, int64_t k, bool &nonfinite)
{
    constexpr int N = VEC4 ? 4 : 1;
    int gc;
    if (!locate_cell(P, x, y, z, gc)) {
        const float qnan = __int_as_float(0x7fc00000);
        if (VEC4) ((float4 *)a.out)[k] = make_float4(qnan, qnan, qnan, qnan);
        else ((float *)a.out)[k] = qnan;
        return SH_OUTSIDE;
    }
    const DepAxis a1(-y, a), a2(x, a), a3(-z, a);
    const int M = a.M;
    // the voxels the point reaches on each axis: a weight of exactly 0 is no voxel (n0 + 1 == M always has one)
    const bool r1[2] = {a1.w0 != 0.f, a1.w1 != 0.f && a1.n0 + 1 < M}, r2[2] = {a2.w0 != 0.f, a2.w1 != 0.f && a2.n0 + 1 < M},
               r3[2] = {a3.w0 != 0.f, a3.w1 != 0.f && a3.n0 + 1 < M};
    const float w1[2] = {a1.w0, a1.w1}, w2[2] = {a2.w0, a2.w1}, w3[2] = {a3.w0, a3.w1};
    float v[8][N];
    // the loads: four rows (d3, d1), every one issued before any is used
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int d3 = r >> 1, d1 = r & 1;
        const bool row = r3[d3] && r1[d1];
        const int64_t at = ((int64_t)(a3.n0 + d3) * M + (a1.n0 + d1)) * M + a2.n0;
#pragma unroll
        for (int c = 0; c < N; c++) v[2 * r][c] = v[2 * r + 1][c] = 0.f;
        if (VEC4) {
            const float4 *f = (const float4 *)a.field + at;
            if (row && r2[0]) { const float4 q = f[0]; v[2 * r][0] = q.x; v[2 * r][1 % N] = q.y; v[2 * r][2 % N] = q.z; v[2 * r][3 % N] = q.w; }
            if (row && r2[1]) { const float4 q = f[1]; v[2 * r + 1][0] = q.x; v[2 * r + 1][1 % N] = q.y; v[2 * r + 1][2 % N] = q.z; v[2 * r + 1][3 % N] = q.w; }
        } else {
            const float *f = (const float *)a.field + at;
            if (row && r2[0] && r2[1]) { const SamplePair q = *(const SamplePair *)f; v[2 * r][0] = q.lo; v[2 * r + 1][0] = q.hi; }
            else if (row && r2[0]) v[2 * r][0] = f[0];
            else if (row && r2[1]) v[2 * r + 1][0] = f[1];
        }
    }
    // the terms, in the deposit's loop order; one fp64 chain per component from +0
    double sum[N];
#pragma unroll
    for (int c = 0; c < N; c++) sum[c] = 0.0;
#pragma unroll
    for (int d3 = 0; d3 < 2; d3++)
#pragma unroll
        for (int d1 = 0; d1 < 2; d1++)
#pragma unroll
            for (int d2 = 0; d2 < 2; d2++) {
                const float W = __fmul_rn(__fmul_rn(w1[d1], w2[d2]), w3[d3]);
                if (r3[d3] && r1[d1] && r2[d2]) {
#pragma unroll
                    for (int c = 0; c < N; c++) sum[c] += (double)__fmul_rn(W, v[(d3 * 2 + d1) * 2 + d2][c]);
                }
            }
    float o[N];
    bool bad = false;
#pragma unroll
    for (int c = 0; c < N; c++) { o[c] = __fmul_rn(a.scale, (float)sum[c]); bad |= !dep_finite(o[c]); }
    if (VEC4) ((float4 *)a.out)[k] = make_float4(o[0], o[1 % N], o[2 % N], o[3 % N]);
    else ((float *)a.out)[k] = o[0];
    nonfinite = bad;
    return SH_SERVED;
}

// a wave's counts, every lane of it calling: oc < 0: the lane had no entry
struct SampleCounts {
    int served = 0, outside = 0, nonfinite = 0;
    __device__ __forceinline__ void add(int oc, bool nf)
    {
        served += __popcll(__ballot(oc == SH_SERVED)); outside += __popcll(__ballot(oc == SH_OUTSIDE)); nonfinite += __popcll(__ballot(nf));
    }
    __device__ __forceinline__ void leave(int lane, int *__restrict__ hdr) const
    {
        if (lane != 0) return;
        if (served) atomicAdd(&hdr[SH_SERVED], served);
        if (outside) atomicAdd(&hdr[SH_OUTSIDE], outside);
        if (nonfinite) atomicAdd(&hdr[SH_NONFINITE], nonfinite);
    }
};

template <bool VEC4>
__global__ __launch_bounds__(SAMPLE_THREADS) void k_sample(DevParams P, const SampleArgs a, int *__restrict__ hdr)
{
    const int n = entry_count(a.count_dev, a.max_count);
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * SAMPLE_THREADS;
    SampleCounts cnt;
    // (a wave's 64 entries are consecutive and its bound is the wave's: every lane reaches the ballots)
    for (int64_t base = (int64_t)blockIdx.x * SAMPLE_THREADS + (threadIdx.x & ~63); base < n; base += stride) {
        const int64_t k = base + lane;
        int oc = -1;
        bool nf = false;
        if (k < n) {
            const float4 p = a.pos4[k];
            oc = sample_entry<VEC4>(P, a, p.x, p.y, p.z, k, nf);
            if (a.outcome) a.outcome[k] = oc;
        }
        cnt.add(oc, nf);
    }
    cnt.leave(lane, hdr);
}

// slot i is live (past the owned slots: not); the load has no branch around it, so a run of them is in flight together
__device__ __forceinline__ bool sample_slot_live(const DevParams &P, const int *__restrict__ cell, int i)
{
    const int c = cell[min(i, P.slots_total - 1)];
    return i < P.slots_total && slot_live(P, c);
}

template <bool VEC4>
__global__ __launch_bounds__(SLOT_THREADS) void k_sample_order(DevParams P, const SampleArgs a, const int *__restrict__ cell,
                                                               const int *__restrict__ tile_live, const float4 *__restrict__ d_pos4,
                                                               int *__restrict__ hdr)
{
    const int n = entry_count(a.count_dev, a.max_count);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x;
    const int before = tiles_before(tile_live, t);        // the live particles of the tiles before this one
    const int first = slot_first(t, wv, lane);
    bool lv[SLOT_ITEMS];
#pragma unroll
    for (int k = 0; k < SLOT_ITEMS; k++) lv[k] = sample_slot_live(P, cell, first + 64 * k);
    int live = 0;
#pragma unroll
    for (int k = 0; k < SLOT_ITEMS; k++) live += __popcll(__ballot(lv[k]));
    int at = __builtin_amdgcn_readfirstlane(wave_offset<int>(before, live, wv, lane));
    SampleCounts cnt;
    // (live particles past n are not served: once the wave's next entry is at or past n, the rest of its slots are too)
#pragma unroll 1
    for (int k0 = 0; k0 < SLOT_ITEMS && at < n; k0 += SAMPLE_BATCH) {
        int e[SAMPLE_BATCH];
        float4 p[SAMPLE_BATCH];
        unsigned long long m[SAMPLE_BATCH];
#pragma unroll
        for (int k = 0; k < SAMPLE_BATCH; k++) m[k] = __ballot(sample_slot_live(P, cell, first + 64 * (k0 + k)));
#pragma unroll
        for (int k = 0; k < SAMPLE_BATCH; k++) {
            e[k] = ((m[k] >> lane) & 1ull) ? at + lane_rank(m[k]) : INT_MAX;
            at += __popcll(m[k]);
            p[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e[k] < n) p[k] = d_pos4[first + 64 * (k0 + k)];
        }
#pragma unroll
        for (int k = 0; k < SAMPLE_BATCH; k++) {
            int oc = -1;
            bool nf = false;
            if (e[k] < n) {
                oc = sample_entry<VEC4>(P, a, p[k].x, p[k].y, p[k].z, e[k], nf);
                if (a.outcome) a.outcome[e[k]] = oc;
            }
            cnt.add(oc, nf);
        }
    }
    cnt.leave(lane, hdr);
}

__global__ void k_sample_finish(const int *__restrict__ hdr, psamd_sample_result *own, psamd_sample_result *out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    psamd_sample_result res;
    res.served = hdr[SH_SERVED]; res.outside = hdr[SH_OUTSIDE]; res.nonfinite = hdr[SH_NONFINITE];
    res.done = res.served + res.outside;                  // every entry examined has one of the two outcomes
    write_result(own, out, res);
}

hipError_t launch_sample(hipStream_t st, const DevParams &P, const DeviceState &d, const SampleArgs &a, const SampleScratch &s,
                         int *tile_live)
{
    {   const hipError_t e = hipMemsetAsync(s.hdr, 0, SAMPLE_HDR_WORDS * sizeof(int), st); if (e != hipSuccess) return e; }
    const bool vec4 = (a.flags & PSAMD_SAMPLE_VEC4) != 0;
    if (a.flags & PSAMD_SAMPLE_EXPORT_ORDER) {
        const int ntiles = slot_tiles(P.slots_total);
        {   const hipError_t e = launch_live_tiles(st, P, d, tile_live); if (e != hipSuccess) return e; }
        if (ntiles > 0) {
            if (vec4) k_sample_order<true><<<ntiles, SLOT_THREADS, 0, st>>>(P, a, d.cell, tile_live, d.pos4, s.hdr);
            else k_sample_order<false><<<ntiles, SLOT_THREADS, 0, st>>>(P, a, d.cell, tile_live, d.pos4, s.hdr);
            PS_LAUNCH_CHECK();
        }
    } else {
        const int blocks = blocks_for((size_t)a.max_count, SAMPLE_THREADS, SAMPLE_MAX_BLOCKS);
        if (vec4) k_sample<true><<<blocks, SAMPLE_THREADS, 0, st>>>(P, a, s.hdr);
        else k_sample<false><<<blocks, SAMPLE_THREADS, 0, st>>>(P, a, s.hdr);
        PS_LAUNCH_CHECK();
    }
    k_sample_finish<<<1, 64, 0, st>>>(s.hdr, s.own, a.result);
    PS_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace psamd
