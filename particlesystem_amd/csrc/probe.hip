// probe.hip -- psamd_probe: the acceleration and the potential of the frame's field at points of the caller's choosing.
//
// Not part of the step and not in the reference.  A probe is no particle: it has a position and
// nothing else.  A probe in compute cell c -- a cell this context's force pass walks -- sees exactly the bodies that pass
// walks for c: the 27-cell stencil in the reference's order, of each cell the first min(count, MAX_PARTICLES_PER_CELL)
// entries of the sorted snapshot with their w_eff; an all-pairs context (world 1) goes on over every other cell of the
// box in global index order.  Six enqueues that nothing in between has to wait for:
//   (memset)         the per-cell counters and the four header words
//   k_probe_locate   one lane per entry: locate_cell, the outcome, the local cell; the cell's counter + 1 (an integer
//                    atomic: nothing about a probe's result depends on where it lands in its cell's run); the entries that
//                    are not served get their NaN words here, every entry its outcome
//   k_probe_scan     one workgroup: the counters' exclusive prefix, in place
//   k_probe_scatter  the served entries' indices into cell-major order
//   k_probe_pairs    one wave per 64 consecutive entries of that order, one probe to a lane.  The wave takes the
//                    distinct cells among its lanes one after the other; for each, ALL lanes walk that cell's stencil --
//                    the bodies are wave-uniform (scalar) loads of the four planes, eight to a group, as in force.hip and
//                    potential.hip -- and the lanes that belong to the cell store their four words at the end.  (No lane
//                    is switched off during a walk: the stencil lookup (stencil_ranges) is handed out by readlane, and
//                    a lane of another cell only computes numbers nobody keeps.)
//   k_probe_finish   the result record
//
// Acceleration: one fp32 chain per component from +0, every body added in list order by the context's own pair form
// (pair_math.hpp, acc_walk).  On the lean exact path a probe on an adult of a cutoff context
// repeats that particle's force chain operation for operation: the same bits as its force record (the own term is r * s
// with r = 0).  Potential: pot_walk.hpp, potential.hip's association unchanged.  All-pairs: each far cell's terms in fp32
// chains of at most POT_CHAIN that start at +0 with the cell and are carried on in fp64, a = (float)((double)a_stencil +
// far) -- NOT the force pass's far-field association (allpairs.hip: 16 partial sums), so equality with the force record
// is promised for cutoff contexts only; with empty far cells the result is the cutoff result bit for bit.
//
// PSAMD_PROBE_FAR (far-field contexts, flat or as a pyramid): the moments are formed first, by the pair stage's own
// kernels (launch_far_moments); behind the stencil a cell's turn goes on over its far set (far_walk.hpp: levels, blocks and
// members are the force pass's) -- a function of the one cell being walked, so members and masks are scalar.  The
// acceleration IS the force pass's association (farfield.hip): a block of 64 level cells goes through the same
// far_block_chain -- every member through the context's pair form, eight level cells to a call with the others entered at
// mass 0, one chain from +0 -- the block sums into the level's sum (flat: into the 16 parts) from +0, those added to the
// stencil's chain top level first (part 0 first): on the exact path a probe on a served adult returns its force record
// bit for bit.  phi: pot_far_block over the same blocks, psamd_potential's.
//
// PSAMD_PROBE_FAR | PSAMD_PROBE_QUADRUPOLE (quadrupole contexts): the acceleration is k_far_walk<.., true, true>'s association
// -- far_quad_group as far_block_chain's `after` hook: a block's quadrupole chain from +0 behind each group's pair terms, the
// blocks' quadrupole chains added in block order to +0, the level's part RN(monopole sum + quadrupole sum) -- and phi is
// psamd_potential's quadrupole form: behind a block's monopole chain its quadrupole chain, each carried into the fp64 sum by
// its own addition.  Where both are asked for, a body's front (far_walk.hpp, far_quad_front) is formed once, in the
// acceleration's walk, and phi's chain rides along: the same terms in the same order as the walk of its own.
//
// The kernel is templated on acc / phi / both, generic exact / lean exact / fast, cutoff / all-pairs / far monopoles / quadrupoles; the
// registers and waves per SIMD of every instance are in the table at k_probe_pairs.
#include "far_walk.hpp"
#include "multisplit.hpp"
#include "pot_walk.hpp"

namespace psamd {

constexpr int PROBE_THREADS = 256;
constexpr int PROBE_OUTSIDE = -2, PROBE_FOREIGN = -3;      // an entry's code: its local cell, or -1 - outcome
enum { PH_NONFINITE = 0, PH_SERVED, PH_OUTSIDE, PH_FOREIGN };   // the header words behind the counters (PROBE_HDR_WORDS)

// a cell this context's force pass walks (the whole pair stage's ranges: lent-in layers, the own computed cells)
__device__ __forceinline__ bool probe_computes(const DevParams &P, int lc)
{
    return (lc >= P.comp_lo[0] && lc < P.comp_hi[0]) || (lc >= P.comp_lo[1] && lc < P.comp_hi[1]) ||
           (lc >= P.comp_lo[2] && lc < P.comp_hi[2]);
}

__global__ __launch_bounds__(PROBE_THREADS) void k_probe_locate(DevParams P, const float4 *__restrict__ pos4, int64_t max_count,
                                                                const int64_t *count_dev, int *__restrict__ code,
                                                                int *__restrict__ counts, int *__restrict__ hdr,
                                                                float4 *__restrict__ out4, int *__restrict__ outcome)
{
    const int n = entry_count(count_dev, max_count);
    const int64_t i64 = (int64_t)blockIdx.x * PROBE_THREADS + threadIdx.x;
    int oc = -1;
    if (i64 < n) {
        const int i = (int)i64;
        const float4 p = pos4[i];
        int gc, lc = PROBE_OUTSIDE;
        if (locate_cell(P, p.x, p.y, p.z, gc)) {
            lc = local_of_global(P, gc);
            if (lc < 0 || !probe_computes(P, lc)) lc = PROBE_FOREIGN;
        }
        code[i] = lc;
        oc = lc >= 0 ? 0 : -1 - lc;
        if (lc >= 0) atomicAdd(&counts[lc], 1);
        else {
            const float qnan = __int_as_float(0x7fc00000);
            out4[i] = make_float4(qnan, qnan, qnan, qnan);
        }
        if (outcome) outcome[i] = oc;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int cnt = __popcll(__ballot(oc == k));
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&hdr[PH_SERVED + k], cnt);
    }
}

// one workgroup: counts[c] becomes the number of served entries in the cells before c
__global__ __launch_bounds__(1024) void k_probe_scan(int ncells, int *__restrict__ counts)
{
    __shared__ int s_w[16];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int run = 0;
    for (int b = 0; b < ncells; b += 1024) {
        const int c = b + tid;
        const int v = c < ncells ? counts[c] : 0;
        const int incl = wave_incl_scan(v);
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) { if (k < wv) before += s_w[k]; total += s_w[k]; }
        if (c < ncells) counts[c] = run + before + incl - v;
        run += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(PROBE_THREADS) void k_probe_scatter(int64_t max_count, const int64_t *count_dev,
                                                                 const int *__restrict__ code, int *__restrict__ counts,
                                                                 int *__restrict__ order)
{
    const int n = entry_count(count_dev, max_count);
    const int64_t i64 = (int64_t)blockIdx.x * PROBE_THREADS + threadIdx.x;
    if (i64 >= n) return;
    const int lc = code[(int)i64];
    if (lc >= 0) order[atomicAdd(&counts[lc], 1)] = (int)i64;      // (below the served count, which is at most n <= the scratch's room)
}

__device__ __forceinline__ bool probe_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// VGPRs / waves per SIMD as the compiler reports them for gfx950, no instance with scratch (cutoff | all-pairs | far
// monopoles | quadrupoles; the generic exact form has no all-pairs, far-monopole or quadrupole instance):
//                 generic exact      lean exact                      fast
//   acc           28 / 8             66 / 7 | 83 / 5 | 79 / 6 | 134 / 3      58 / 8 | 75 / 6 | 71 / 7 | 114 / 4
//   phi           40 / 7             40 / 7 | 41 / 7 | 41 / 7 | 47 / 7       40 / 7 | 41 / 7 | 41 / 7 | 47 / 7
//   acc and phi   44 / 7             72 / 7 | 87 / 5 | 83 / 5 | 135 / 3      62 / 7 | 77 / 6 | 73 / 6 | 115 / 4
// (acc and phi walk a cell's list once each: the two passes share no registers, and their loads hit the scalar cache.  The
// quadrupole instances with acc carry a group's pair rows and its ten planes at once; the report shows 55-83 scalar registers
// kept in vector lanes and no scratch, so they keep the others' launch bound -- by that report, not by a timing.)
template <int FIELDS, int MATH, int FAR>      // FAR 0: the stencil alone; 1: all-pairs; 2: far monopoles, flat or as a pyramid; 3: ... and their quadrupole terms
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_pairs(DevParams P, const int *__restrict__ cell_start,
                                                               const float *__restrict__ snap_soa,
                                                               const float4 *__restrict__ pos4, const int *__restrict__ code,
                                                               const int *__restrict__ order, int *__restrict__ hdr,
                                                               const PotFar far, const FarMoments mono, float4 *__restrict__ out4)
{
    // waves of 64 consecutive served entries, four independent waves per workgroup, an XCD's workgroups a contiguous run
    // of the cell-major order (force.hip, k_pairs).  The launch is sized by max_count, the work by the served count.
    const int lane = threadIdx.x & 63;
    const int served = hdr[PH_SERVED];
    const int nwave = (int)(((int64_t)served + 63) >> 6), nwg = (nwave + 3) >> 2;
    if ((int)blockIdx.x >= nwg) return;
    const int slot = __builtin_amdgcn_readfirstlane(xcd_contiguous(blockIdx.x, nwg) * 4 + (int)(threadIdx.x >> 6));
    if (slot >= nwave) return;
    const int64_t j = (int64_t)slot * 64 + lane;
    const bool valid = j < served;
    const int i = valid ? order[j] : 0;
    const int lc = valid ? code[i] : -1;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid) p = pos4[i];
    const size_t cap = (size_t)P.sorted_cap;
    const float eps2f = (float)P.eps2;
    const PairCtx ctx = {p.x, p.y, p.z, 0.f, 0, -1, false};
    int nonfinite = 0;
    for (unsigned long long todo = __ballot(valid); todo;) {
        const int first = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        const int c = __builtin_amdgcn_readlane(lc, first);
        const unsigned long long mine = __ballot(valid && lc == c);
        todo &= ~mine;
        int i1, i2, i3;
        cell_coords(P, c, i1, i2, i3);
        int my_nb, my_cnt;
        stencil_ranges(P, cell_start, i1, i2, i3, lane, my_nb, my_cnt);
        float ax = 0.f, ay = 0.f, az = 0.f;
        double acc = 0.0;
        for (int k = 0; k < STENCIL; k++) {                 // the stencil, in the reference's order
            const int nb = __builtin_amdgcn_readlane(my_nb, k), n = __builtin_amdgcn_readlane(my_cnt, k);
            const float *sx = snap_soa + nb;
            if (FIELDS & PSAMD_PROBE_ACC) acc_walk<MATH, 8>(P, ctx, sx, sx + cap, sx + 2 * cap, sx + 3 * cap, n, eps2f, ax, ay, az);
            if (FIELDS & PSAMD_PROBE_PHI) pot_walk<false>(ctx, sx, sx + cap, sx + 2 * cap, sx + 3 * cap, n, 0, eps2f, true, acc);
        }
        if (FAR >= 2) {
            // the far set of THIS cell (world == 1: local cell == global cell), levels top down; a level's blocks in index
            // order, dealt to the force pass's parts (one part a level on a pyramid)
            constexpr bool QUAD = FAR == 3, ACC = (FIELDS & PSAMD_PROBE_ACC) != 0, PHI = (FIELDS & PSAMD_PROBE_PHI) != 0;
            for (int l = mono.nlev - 1; l >= 0; l--) {
                const FarLevelView v = far_level_view(mono, l, i1, i2, i3);
                for (int part = 0; part < mono.nparts; part++) {
                    const int b_lo = max(v.blk_lo, v.lev.nblk * part / mono.nparts), b_hi = min(v.blk_hi, v.lev.nblk * (part + 1) / mono.nparts);
                    float px = 0.f, py = 0.f, pz = 0.f;     // the part's sum
                    float ux = 0.f, uy = 0.f, uz = 0.f;     // ... and its quadrupole sum (QUAD)
                    for (int blk = b_lo; blk < b_hi; blk++) {
                        const unsigned long long take = far_members(mono, v, blk, lane);
                        if (take == 0ull) continue;         // (a chain of nothing is +0, and neither sum ever is -0)
                        const float *sx = mono.mom + v.lev.off + blk * 64, *sy = sx + mono.mom_cap, *sz = sy + mono.mom_cap, *sw = sz + mono.mom_cap;
                        float bp = 0.f;                     // the block's quadrupole chain of phi, where the acceleration's walk forms it
                        if (ACC) {
                            // the force pass's chain for the block; what a cell of a group is left out by is a scalar mask here
                            float cx, cy, cz;
                            const auto leave = [&](int g, v2f (&qw)[4]) {
#pragma unroll
                                for (int k = 0; k < 8; k++) far_drop(qw, k, !((take >> (g + k)) & 1ull));
                            };
                            if (QUAD) {
                                // ... and the force pass's quadrupole chain behind each group's pair terms; with PHI the
                                // potential's quadrupole chain from the same front of every body
                                float bx = 0.f, by = 0.f, bz = 0.f;
                                const float *sc = sw + mono.mom_cap;
                                far_block_chain<MATH>(P, ctx, sx, sy, sz, sw, take, eps2f, leave, [&](int g, v2f (&qx)[4], v2f (&qy)[4], v2f (&qz)[4], v2f (&qw)[4]) {
                                    far_quad_group<true, PHI>(ctx, qx, qy, qz, qw, sc + g, mono.mom_cap, eps2f, bx, by, bz, bp);
                                }, cx, cy, cz);
                                ux = __fadd_rn(ux, bx); uy = __fadd_rn(uy, by); uz = __fadd_rn(uz, bz);
                            } else far_block_chain<MATH>(P, ctx, sx, sy, sz, sw, take, eps2f, leave, cx, cy, cz);
                            px += cx; py += cy; pz += cz;
                        }
                        if (PHI) {
                            pot_far_block(ctx, sx, sy, sz, sw, take, eps2f, acc);
                            if (QUAD && ACC) acc += (double)bp;
                            else if (QUAD) far_quad_phi_block(ctx, sx, sy, sz, sw + mono.mom_cap, mono.mom_cap, take, eps2f, acc);
                        }
                    }
                    if (ACC && QUAD) { px = __fadd_rn(px, ux); py = __fadd_rn(py, uy); pz = __fadd_rn(pz, uz); }
                    if (ACC) { ax += px; ay += py; az += pz; }
                }
            }
        }
        if (FAR == 1) {
            // every other cell of the box in global index order (k_pot_pairs<1>'s walk); the cells of THIS cell's
            // stencil are left out for this cell's turn
            const size_t plane = (size_t)far.plane;
            const int nblk = (P.num_cells_global + 63) >> 6;
            double fx = 0.0, fy = 0.0, fz = 0.0;
            for (int blk = 0; blk < nblk; blk++) {
                const int c2 = blk * 64 + lane;
                int f_nb = 0, f_cnt = 0;
                if (c2 < P.num_cells_global) {
                    int j1, j2, j3;
                    global_coords(P, c2, j1, j2, j3);
                    f_nb = far.start[c2];
                    f_cnt = far.n ? far.n[c2] : min(far.start[c2 + 1] - f_nb, P.max_per_cell);
                    if (abs(j3 - i3) <= 1 && abs(j1 - i1) <= 1 && abs(j2 - i2) <= 1) f_cnt = 0;
                }
                for (unsigned long long ft = __ballot(f_cnt > 0); ft; ft &= ft - 1) {
                    const int q = __builtin_amdgcn_readfirstlane(__ffsll((long long)ft) - 1);
                    const int nb = __builtin_amdgcn_readlane(f_nb, q), n = __builtin_amdgcn_readlane(f_cnt, q);
                    const float *sx = far.buf + nb;
                    if (FIELDS & PSAMD_PROBE_ACC) {
                        for (int j0 = 0; j0 < n; j0 += POT_CHAIN) {
                            float cx = 0.f, cy = 0.f, cz = 0.f;
                            acc_walk<MATH, 8>(P, ctx, sx + j0, sx + plane + j0, sx + 2 * plane + j0, sx + 3 * plane + j0,
                                              min(POT_CHAIN, n - j0), eps2f, cx, cy, cz);
                            fx += (double)cx; fy += (double)cy; fz += (double)cz;
                        }
                    }
                    if (FIELDS & PSAMD_PROBE_PHI)
                        pot_walk<false>(ctx, sx, sx + plane, sx + 2 * plane, sx + 3 * plane, n, 0, eps2f, far.padded != 0, acc);
                }
            }
            if (FIELDS & PSAMD_PROBE_ACC) {
                ax = (float)((double)ax + fx); ay = (float)((double)ay + fy); az = (float)((double)az + fz);
            }
        }
        if ((mine >> lane) & 1ull) {
            const float phi = (FIELDS & PSAMD_PROBE_PHI) ? (float)(-acc) : 0.f;
            out4[i] = make_float4(ax, ay, az, phi);          // (components not asked for were never touched: 0)
            if (!(probe_finite(ax) && probe_finite(ay) && probe_finite(az) && probe_finite(phi))) nonfinite = 1;
        }
    }
    const int cnt = __popcll(__ballot(nonfinite != 0));
    if (lane == 0 && cnt) atomicAdd(&hdr[PH_NONFINITE], cnt);
}

__global__ void k_probe_finish(int64_t max_count, const int64_t *count_dev, const int *__restrict__ hdr,
                               psamd_probe_result *own, psamd_probe_result *out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    psamd_probe_result res;
    res.done = entry_count(count_dev, max_count);
    res.served = hdr[PH_SERVED]; res.outside = hdr[PH_OUTSIDE]; res.foreign = hdr[PH_FOREIGN]; res.nonfinite = hdr[PH_NONFINITE];
    write_result(own, out, res);
}

template <int FIELDS, int MATH>
static void launch_probe_pairs(hipStream_t st, const DevParams &P, const DeviceState &d, const ProbeArgs &a, const ProbeScratch &s,
                               int *hdr, unsigned nwg)
{
    const bool far_form = (a.fields & (PSAMD_PROBE_FAR | PSAMD_PROBE_QUADRUPOLE)) != 0, allp = !far_form && (P.flags & PSAMD_FLAG_ALL_PAIRS);
    const auto launch = [&](auto kernel) {
        kernel<<<nwg, PROBE_THREADS, 0, st>>>(P, d.cell_start, d.snap_soa, a.pos4, s.code, s.order, hdr, allp ? pot_far_of(P, d, false) : PotFar{},
                                              far_form ? far_moments_of(P, d) : FarMoments{}, a.out4);
    };
    // (quadrupole contexts are far-monopole contexts, and the bit comes with PSAMD_PROBE_FAR; far-monopole and all-pairs contexts
    // are created only with lean arithmetic, and probed on world 1 only: the own snapshot)
    if constexpr (MATH != 0) {
        if (a.fields & PSAMD_PROBE_QUADRUPOLE) return launch(k_probe_pairs<FIELDS, MATH, 3>);
        if (a.fields & PSAMD_PROBE_FAR) return launch(k_probe_pairs<FIELDS, MATH, 2>);
        if (allp) return launch(k_probe_pairs<FIELDS, MATH, 1>);
    }
    if (!far_form && !allp) launch(k_probe_pairs<FIELDS, MATH, 0>);
}

template <int FIELDS>
static void launch_probe_fields(hipStream_t st, const DevParams &P, const DeviceState &d, const ProbeArgs &a, const ProbeScratch &s,
                                int *hdr, unsigned nwg)
{
    if (!P.lean_math) launch_probe_pairs<FIELDS, 0>(st, P, d, a, s, hdr, nwg);
    else if (P.flags & PSAMD_FLAG_FAST_MATH) launch_probe_pairs<FIELDS, 2>(st, P, d, a, s, hdr, nwg);
    else launch_probe_pairs<FIELDS, 1>(st, P, d, a, s, hdr, nwg);
}

hipError_t launch_probe(hipStream_t st, const DevParams &P, const DeviceState &d, const ProbeArgs &a, const ProbeScratch &s)
{
    const int ncells = P.n_local_cells;
    int *hdr = s.counts + ncells + 1;
    if (a.fields & PSAMD_PROBE_FAR) { launch_far_moments(st, P, d); PS_LAUNCH_CHECK(); }
    {   const hipError_t e = hipMemsetAsync(s.counts, 0, (size_t)(ncells + 1 + PROBE_HDR_WORDS) * sizeof(int), st); if (e != hipSuccess) return e; }
    const unsigned blocks = (unsigned)((a.max_count + PROBE_THREADS - 1) / PROBE_THREADS);
    k_probe_locate<<<blocks, PROBE_THREADS, 0, st>>>(P, a.pos4, a.max_count, a.count_dev, s.code, s.counts, hdr, a.out4, a.outcome);
    PS_LAUNCH_CHECK();
    k_probe_scan<<<1, 1024, 0, st>>>(ncells, s.counts);
    PS_LAUNCH_CHECK();
    k_probe_scatter<<<blocks, PROBE_THREADS, 0, st>>>(a.max_count, a.count_dev, s.code, s.counts, s.order);
    PS_LAUNCH_CHECK();
    const unsigned nwg = (unsigned)((a.max_count + 255) / 256);
    const uint32_t what = a.fields & (PSAMD_PROBE_ACC | PSAMD_PROBE_PHI);      // (PSAMD_PROBE_FAR and PSAMD_PROBE_QUADRUPOLE are modifiers)
    if (what == PSAMD_PROBE_ACC) launch_probe_fields<PSAMD_PROBE_ACC>(st, P, d, a, s, hdr, nwg);
    else if (what == PSAMD_PROBE_PHI) launch_probe_fields<PSAMD_PROBE_PHI>(st, P, d, a, s, hdr, nwg);
    else launch_probe_fields<PSAMD_PROBE_ACC | PSAMD_PROBE_PHI>(st, P, d, a, s, hdr, nwg);
    PS_LAUNCH_CHECK();
    k_probe_finish<<<1, 64, 0, st>>>(a.max_count, a.count_dev, hdr, s.own, a.result);
    PS_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace psamd
