// potential.hip -- psamd_potential: every listed particle's potential and the potential energy, on the device.
//
// Not part of the step and not in the reference.  The pass reads the frame psamd_build_grid left
// (cell_start, sorted_id, the snap_soa planes) and walks, for every particle of the own cells' lists, exactly the
// bodies the force pass walks for its cell:
//   phi_i = - sum over j != i of w_j / sqrt(|x_j - x_i|^2 + eps2)        (w_j: the snapshot's w_eff -- force_sign is
//                                                                         in it, a kid's is 0)
//   U     = 1/2 sum_i |w_i| phi_i                                        (fp64)
// in three launches that nothing in between has to wait for:
//   k_pot_pairs   one wave per (own cell, 64-particle slice), one lane per particle: the 27-cell stencil in the
//                 reference's order, the bodies as wave-uniform (scalar) loads of the four planes, eight to a group in
//                 pair_math.hpp's packed forms; all-pairs contexts go on over every other cell in global order, far-
//                 field contexts asked with PSAMD_POTENTIAL_FAR over the cell's far set (far_walk.hpp).  The
//                 lane's own entry is left out BY SORTED INDEX: two particles at one point see each other.
//                 phi by sorted index.
//   k_pot_reduce  per tile of POT_TILE sorted entries: phi scattered to slot order through sorted_id; U, the extrema and
//                 the counts of the tile in a fixed tree; and -- tile t of the owned SLOTS -- its live count.
//   k_pot_finish  workgroup 0: the tiles in index order, the result record; workgroup 1 + t: slot tile t of phi
//                 compacted to export order (ascending slot id: entry k pairs with psamd_export_live's entry k).
// The launch boundaries are the only ordering between the workgroups; the walk over the owned slots is slot_walk.hpp's.
//
// Accumulation.  Terms are fp32 (differences and r.r as the force pass forms them, v_rsq_f32, one multiply).  They are
// added in list order in fp32 CHAINS of at most POT_CHAIN terms; a chain starts at +0 with every cell (and every
// POT_CHAIN bodies inside a cell) and its sum is carried on in fp64.  A particle's association therefore depends on
// nothing but the cell order and the cells' list lengths: the same bits from run to run, with graphs or without, on one
// context and on the slab that holds the particle.  Against an fp64 direct sum: 1.5e-7 relative for phi, 1e-8 for U
// (tests/test_gpu_potential.py prints the largest error of every case).
//
// PSAMD_POTENTIAL_FAR (far-field contexts, flat or as a pyramid): the moments are formed first, by the pair stage's own
// kernels from the same snapshot (launch_far_moments: the same bits in the same buffers, whether the pair stage has run or
// not); behind the stencil's chains come the levels top down (flat: the one level), of each level the blocks of 64 cells in
// index order, a block's members one chain from +0 (pot_far_walk).  Levels, blocks and members are far_walk.hpp's, the ones
// the force pass walks; the set is a function of the wave's one cell: members and masks are scalar.
//
// PSAMD_POTENTIAL_FAR | PSAMD_POTENTIAL_QUADRUPOLE (quadrupole contexts): all of the above bit for bit, and behind every
// block's monopole chain that block's quadrupole chain -- the members' terms t_q = 1.5 (d.C.d) u^5 - 0.5 T u^3 (far_walk.hpp,
// far_quad_phi: the force term's front), one fp32 chain from +0 in index order, carried into the fp64 sum by an addition of
// its own.
//
// VGPRs / waves per SIMD of k_pot_pairs as the compiler reports them for gfx950, no instance with scratch:
//   cutoff 40 / 8      all-pairs 44 / 8      far monopoles 42 / 8      quadrupoles 43 / 7
// (the quadrupole instance holds a group's X, Y, Z and six C planes in scalar registers: the report shows 32 of them kept in
// vector lanes and no scratch, so it keeps the launch bound of the others -- by that report, not by a timing)
#include "far_walk.hpp"
#include "pot_walk.hpp"
#include "slot_walk.hpp"

namespace psamd {

constexpr int POT_THREADS = SLOT_THREADS, POT_WAVES = SLOT_WAVES;   // (k_pot_reduce walks tile t of the sorted order and of the slots)
constexpr int POT_ITEMS = POT_TILE / POT_THREADS;        // 16 batches of 64 entries per wave
static_assert(POT_ITEMS == SLOT_ITEMS, "a wave walks POT_ITEMS batches of 64 sorted entries and as many of 64 slots");

__device__ __forceinline__ bool pot_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// The far part of phi for the cell (i1, i2, i3) all lanes of the wave walk: levels top down, blocks in index order.  QUAD:
// behind a block's monopole chain that block's quadrupole chain, over the same members (the six C planes lie behind the
// four of mom, mom_cap apart: wave-uniform loads like the moments).
template <bool QUAD>
__device__ __forceinline__ void pot_far_walk(const PairCtx &ctx, const FarMoments &m, int i1, int i2, int i3, int lane,
                                             float eps2f, double &acc)
{
    for (int l = m.nlev - 1; l >= 0; l--) {
        const FarLevelView v = far_level_view(m, l, i1, i2, i3);
        for (int blk = v.blk_lo; blk < v.blk_hi; blk++) {
            const unsigned long long take = far_members(m, v, blk, lane);
            if (take == 0ull) continue;
            const float *sx = m.mom + v.lev.off + blk * 64, *sy = sx + m.mom_cap, *sz = sy + m.mom_cap, *sw = sz + m.mom_cap;
            pot_far_block(ctx, sx, sy, sz, sw, take, eps2f, acc);
            if (QUAD) far_quad_phi_block(ctx, sx, sy, sz, sw + m.mom_cap, m.mom_cap, take, eps2f, acc);
        }
    }
}

template <int FAR>      // 0: the stencil alone; 1: all-pairs; 2: far monopoles, flat or as a pyramid; 3: ... and their quadrupole terms
__global__ __launch_bounds__(POT_THREADS) void k_pot_pairs(DevParams P, const int *__restrict__ cell_start,
                                                           const float *__restrict__ snap_soa,
                                                           const float *__restrict__ snap_age,
                                                           const int *__restrict__ sorted_id,
                                                           const float4 *__restrict__ pos4, const PotFar far,
                                                           const FarMoments mono, float *__restrict__ phi_sorted)
{
    // (cell, slice) tasks of every own cell, cell-major; four independent waves per workgroup, an XCD's workgroups a
    // contiguous run of cells (force.hip, k_pairs).  Slices past a cell's count end at once.
    const int lane = threadIdx.x & 63;
    const int ntask = P.n_own_cells * P.slices, nwg = (ntask + 3) >> 2;
    if ((int)blockIdx.x >= nwg) return;
    const int slot = __builtin_amdgcn_readfirstlane(xcd_contiguous(blockIdx.x, nwg) * 4 + (int)(threadIdx.x >> 6));
    if (slot >= ntask) return;
    const int c = slot / P.slices, slice = slot - c * P.slices;
    const int base = cell_start[c];
    const int cnt = min(cell_start[c + 1] - base, P.max_per_cell);
    const int first = slice * 64;
    if (first >= cnt) return;
    const bool valid = lane < min(64, cnt - first);
    const int gi = base + first + (valid ? lane : 0);
    const size_t cap = (size_t)P.sorted_cap;
    float mx = snap_soa[gi], my = snap_soa[cap + gi], mz = snap_soa[2 * cap + gi];
    if (snap_age[gi] < P.kid_thr) {              // a kid's snapshot position is the origin (grid.hip): its own is in its slot
        const int si = slot_index(P, sorted_id[gi]);
        if (si >= 0) { const float4 p = pos4[si]; mx = p.x; my = p.y; mz = p.z; }
    }
    int i1, i2, i3;
    cell_coords(P, c, i1, i2, i3);
    const float eps2f = (float)P.eps2;
    const PairCtx ctx = {mx, my, mz, 0.f, 0, gi, false};
    int my_nb, my_cnt;
    stencil_ranges(P, cell_start, i1, i2, i3, lane, my_nb, my_cnt);
    double acc = 0.0;
    {   // the own cell first, as the stencil has it
        const float *sx = snap_soa + base;
        pot_walk<true>(ctx, sx, sx + cap, sx + 2 * cap, sx + 3 * cap, cnt, base, eps2f, true, acc);
    }
    for (int k = 1; k < STENCIL; k++) {
        const int nb = __builtin_amdgcn_readlane(my_nb, k), n = __builtin_amdgcn_readlane(my_cnt, k);
        const float *sx = snap_soa + nb;
        pot_walk<false>(ctx, sx, sx + cap, sx + 2 * cap, sx + 3 * cap, n, 0, eps2f, true, acc);
    }
    if (FAR >= 2) pot_far_walk<FAR == 3>(ctx, mono, i1, i2, i3, lane, eps2f, acc);      // (world == 1: local cell == global cell)
    if (FAR == 1) {
        // every other cell of the box in global index order, 64 cell ranges to a vector load (allpairs.hip); the wave's
        // particles share one cell, so the cells of its stencil are left out for the whole wave
        const size_t plane = (size_t)far.plane;
        const int nblk = (P.num_cells_global + 63) >> 6;
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
            for (unsigned long long todo = __ballot(f_cnt > 0); todo; todo &= todo - 1) {
                const int q = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
                const int nb = __builtin_amdgcn_readlane(f_nb, q), n = __builtin_amdgcn_readlane(f_cnt, q);
                const float *sx = far.buf + nb;
                pot_walk<false>(ctx, sx, sx + plane, sx + 2 * plane, sx + 3 * plane, n, 0, eps2f, far.padded != 0, acc);
            }
        }
    }
    if (valid) phi_sorted[gi] = (float)(-acc);
}

// What a tile, a wave or a lane has seen of the listed particles.
struct PotAcc {
    double u;
    float lo, hi;
    int listed, nonfinite;
    __device__ __forceinline__ void init() { u = 0.0; lo = __int_as_float(0x7f800000); hi = -lo; listed = 0; nonfinite = 0; }
    __device__ __forceinline__ void add(float w, float phi)
    {
        listed++;
        if (!pot_finite(phi)) { nonfinite++; return; }
        u += 0.5 * (double)fabsf(w) * (double)phi;
        lo = fminf(lo, phi); hi = fmaxf(hi, phi);
    }
    __device__ __forceinline__ void merge(const PotAcc &o)
    {
        u += o.u; lo = fminf(lo, o.lo); hi = fmaxf(hi, o.hi); listed += o.listed; nonfinite += o.nonfinite;
    }
    __device__ __forceinline__ void wave_reduce()          // a butterfly: the same fixed tree on every run
    {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            PotAcc o;
            o.u = __shfl_xor(u, m); o.lo = __shfl_xor(lo, m); o.hi = __shfl_xor(hi, m);
            o.listed = __shfl_xor(listed, m); o.nonfinite = __shfl_xor(nonfinite, m);
            merge(o);
        }
    }
};

// Tile t of the sorted order of the own cells (entries cell_start[0] + t * POT_TILE ...; an entry whose id is -1 was
// ranked past its cell's list capacity: no particle) and tile t of the owned slots.
__global__ __launch_bounds__(POT_THREADS) void k_pot_reduce(DevParams P, const int *__restrict__ cell_start,
                                                            const int *__restrict__ sorted_id,
                                                            const float *__restrict__ snap_soa,
                                                            const float *__restrict__ phi_sorted,
                                                            const int *__restrict__ cell, float *__restrict__ phi_slot,
                                                            PotTile *__restrict__ tiles, int *__restrict__ tile_count)
{
    __shared__ PotAcc s_acc[POT_WAVES];
    __shared__ int s_live[POT_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x;
    const int g0 = cell_start[0], g1 = min(cell_start[P.n_own_cells], P.sorted_cap);
    const int off = t * POT_TILE + wv * 64 * POT_ITEMS + lane;
    const float *sw = snap_soa + 3 * (size_t)P.sorted_cap;
    PotAcc a;
    a.init();
    int live = 0;
#pragma unroll 4
    for (int k = 0; k < POT_ITEMS; k++) {
        const int gi = g0 + off + 64 * k;
        const int id = gi < g1 ? sorted_id[gi] : -1;
        if (id >= 0) {
            const float phi = phi_sorted[gi];
            a.add(sw[gi], phi);
            const int si = slot_index(P, id);
            if (phi_slot && si >= 0) phi_slot[si] = phi;
        }
        live += __popcll(__ballot(slot_live(P, slot_cell(P, cell, off + 64 * k))));
    }
    a.wave_reduce();
    if (lane == 0) { s_acc[wv] = a; s_live[wv] = live; }
    __syncthreads();
    if (threadIdx.x == 0) {
        PotAcc b = s_acc[0];
        int n = s_live[0];
        for (int w = 1; w < POT_WAVES; w++) { b.merge(s_acc[w]); n += s_live[w]; }
        PotTile &r = tiles[t];
        r.u = b.u; r.lo = b.lo; r.hi = b.hi; r.listed = b.listed; r.nonfinite = b.nonfinite;
        tile_count[t] = n;
    }
}

// Workgroup 0: U over the tiles in index order -- one serial fp64 chain (tile_order_sums) -- and the extrema and
// counts, which do not depend on the order.
__device__ __forceinline__ void pot_finish(int ntiles, const PotTile *__restrict__ tiles, const int *__restrict__ tile_count,
                                           psamd_potential_result *__restrict__ result_out, PotOut *__restrict__ own)
{
    __shared__ PotAcc s_acc[POT_WAVES];
    __shared__ long long s_live[POT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    PotAcc a;
    a.init();
    long long live = 0;
    const double sum = tile_order_sums<1>(ntiles, [&](int t, double (&v)[1]) {
        const PotTile r = tiles[t];
        v[0] = r.u;
        a.lo = fminf(a.lo, r.lo); a.hi = fmaxf(a.hi, r.hi); a.listed += r.listed; a.nonfinite += r.nonfinite;
        live += tile_count[t];
    });
    a.wave_reduce();
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) live += __shfl_xor(live, m);
    if (lane == 0) { s_acc[wv] = a; s_live[wv] = live; }
    __syncthreads();
    if (tid == 0) {
        long long listed = 0, nonfinite = 0, n = 0;
        float lo = __int_as_float(0x7f800000), hi = -lo;
        for (int w = 0; w < POT_WAVES; w++) {
            listed += s_acc[w].listed; nonfinite += s_acc[w].nonfinite; n += s_live[w];
            lo = fminf(lo, s_acc[w].lo); hi = fmaxf(hi, s_acc[w].hi);
        }
        psamd_potential_result r;
        r.listed = listed; r.nonfinite = nonfinite; r.potential = sum; r.phi_min = (double)lo; r.phi_max = (double)hi;
        own->result = r; own->live = n;
        if (result_out) *result_out = r;
    }
}

// Workgroup 1 + t: slot tile t of phi to export order (the walk of k_export_write).
__global__ __launch_bounds__(POT_THREADS) void k_pot_finish(DevParams P, int ntiles, const int *__restrict__ cell,
                                                            const float *__restrict__ phi_slot,
                                                            const PotTile *__restrict__ tiles, const int *__restrict__ tile_count,
                                                            float *__restrict__ phi_out, int64_t capacity,
                                                            psamd_potential_result *__restrict__ result_out, PotOut *__restrict__ own)
{
    if (blockIdx.x == 0) { pot_finish(ntiles, tiles, tile_count, result_out, own); return; }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x - 1;
    const int before = tiles_before(tile_count, t);
    const int first = slot_first(t, wv, lane);
    unsigned long long mask[SLOT_ITEMS];
    int live = 0;
#pragma unroll
    for (int k = 0; k < SLOT_ITEMS; k++) {
        mask[k] = __ballot(slot_live(P, slot_cell(P, cell, first + 64 * k)));
        live += __popcll(mask[k]);
    }
    int64_t at = wave_offset<int64_t>(before, live, wv, lane);
    if (at >= capacity) return;
#pragma unroll
    for (int k = 0; k < SLOT_ITEMS; k++) {
        const unsigned long long m = mask[k];
        const int64_t o = at + (int64_t)lane_rank(m);
        at += __popcll(m);
        if (((m >> lane) & 1ull) && o < capacity) phi_out[o] = phi_slot[first + 64 * k];
    }
}

hipError_t launch_potential(hipStream_t st, const DevParams &P, const DeviceState &d, float *phi, int64_t capacity,
                            psamd_potential_result *result_dev, uint32_t flags)
{
    const int ntiles = slot_tiles(P.slots_total);
    const bool want_phi = phi && capacity > 0 && ntiles > 0;
    // a live particle that is in no list of the frame keeps this quiet NaN
    if (want_phi) { const hipError_t e = launch_fill_int(st, reinterpret_cast<int *>(d.pot_slot), 0x7fc00000, (size_t)P.slots_total); if (e != hipSuccess) return e; }
    const int ntask = P.n_own_cells * P.slices;
    if (ntask > 0) {
        const bool far_form = (flags & (PSAMD_POTENTIAL_FAR | PSAMD_POTENTIAL_QUADRUPOLE)) != 0, allp = !far_form && (P.flags & PSAMD_FLAG_ALL_PAIRS);
        if (far_form) { launch_far_moments(st, P, d); PS_LAUNCH_CHECK(); }
        const auto launch = [&](auto kernel) {
            kernel<<<(ntask + 3) / 4, POT_THREADS, 0, st>>>(P, d.cell_start, d.snap_soa, d.snap_age, d.sorted_id, d.pos4, allp ? pot_far_of(P, d, P.world > 1) : PotFar{},
                                                            far_form ? far_moments_of(P, d) : FarMoments{}, d.pot_sorted);
        };
        if (flags & PSAMD_POTENTIAL_QUADRUPOLE) launch(k_pot_pairs<3>);
        else if (flags & PSAMD_POTENTIAL_FAR) launch(k_pot_pairs<2>);
        else if (allp) launch(k_pot_pairs<1>);
        else launch(k_pot_pairs<0>);
        PS_LAUNCH_CHECK();
    }
    if (ntiles > 0) {
        k_pot_reduce<<<ntiles, POT_THREADS, 0, st>>>(P, d.cell_start, d.sorted_id, d.snap_soa, d.pot_sorted, d.cell,
                                                     want_phi ? d.pot_slot : nullptr, d.pot_tiles, d.pot_count);
        PS_LAUNCH_CHECK();
    }
    k_pot_finish<<<want_phi ? ntiles + 1 : 1, POT_THREADS, 0, st>>>(P, ntiles, d.cell, d.pot_slot, d.pot_tiles, d.pot_count, phi, capacity,
                                                                    result_dev, d.pot_out);
    PS_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace psamd
