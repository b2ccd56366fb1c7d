// allpairs.hip -- the far field of the all-pairs forces (PSAMD_FLAG_ALL_PAIRS, not in the reference)
#include "pot_walk.hpp"

namespace psamd {

// ------------------------------------------------------------------ all-pairs forces (PSAMD_FLAG_ALL_PAIRS, not in the reference)
// A particle's acceleration = the stencil's chain, exactly force.hip's cutoff pass (the reference's order), plus every
// other cell of the box in GLOBAL index order.  The far field is 99 % of the work and the same for every particle but
// for the 27 cells it must leave out, so it does not go by (cell, slice) tasks -- whose last slices are mostly empty
// lanes: a quarter of all lanes at 64 particles per cell -- but by DENSE tasks: the particles that need a force, in
// cell order, 64 to a wave whatever their cells.  A wave (dense task, part) walks the cells of its part (a sixteenth
// of the box, by blocks of 64 cells) in chunks of ALLP_CHUNK consecutive cells: a chunk's bodies are ONE chain of
// additions started at +0 (an fp32 sum of a quarter of a million terms in one chain would carry 4e-5 of rounding,
// measured at N = 2^18), the chunk's sum is added to the part's, k_allpairs_combine adds the parts to the stencil's
// chain in part order.  A lane whose own stencil holds a cell of the chunk leaves that cell's bodies out (its sums are
// put back after the cell's walk); a chunk no lane has in its stencil, its cells adjacent in the buffer -- nearly
// all -- is walked in one go, with one ragged tail per chunk instead of one per cell.  The association depends on
// nothing but the global cell order: the same bits on one GPU and on any number of ranks, where far_buf is the
// all-gathered snapshot of all ranks with its index by global cell (k_allg_index) instead of the own snapshot.
constexpr int ALLP_CHUNK = 4;          // (divides 64)

// act_start[j]: how many particles need a force in the pass's cells before its j-th; [comp_count]: in all.  One workgroup.
__global__ __launch_bounds__(1024) void k_allp_prefix(DevParams P, const int *__restrict__ active_count, int *__restrict__ act_start)
{
    __shared__ int wave_tot[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ncomp = comp_count(P), per = (ncomp + 1023) / 1024;
    const int c0 = min(ncomp, tid * per), c1 = min(ncomp, c0 + per);
    int mine = 0;
    for (int j = c0; j < c1; j++) mine += active_count[comp_cell(P, j)];
    const int incl = wave_incl_scan(mine);
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    int run = incl - mine, total = 0;
    for (int k = 0; k < 16; k++) { if (k < wv) run += wave_tot[k]; total += wave_tot[k]; }
    for (int j = c0; j < c1; j++) { act_start[j] = run; run += active_count[comp_cell(P, j)]; }
    if (tid == 0) act_start[ncomp] = total;
}

// the dense order: sorted index and cell of the r-th particle that needs a force.  One wave per cell of the pass.
__global__ __launch_bounds__(256) void k_allp_dense(DevParams P, const int *__restrict__ cell_start, const int *__restrict__ active_list,
                                                    const int *__restrict__ active_count, const int *__restrict__ act_start,
                                                    int *__restrict__ dense_gi, int *__restrict__ dense_cell)
{
    const int j = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= comp_count(P)) return;
    const int c = comp_cell(P, j), base = cell_start[c], n = active_count[c], o = act_start[j];
    for (int i = lane; i < n; i += 64) { dense_gi[o + i] = active_list[base + i]; dense_cell[o + i] = c; }
}

template <int MODE, int NQ>
__global__ __launch_bounds__(256, BALANCED_WAVES) void k_allp_far(DevParams P, const SnapSoa snap4, const int *__restrict__ act_start,
                                                                        const int *__restrict__ dense_gi, const int *__restrict__ dense_cell,
                                                                        const FarCells far, const float *__restrict__ far_buf,
                                                                        const int *__restrict__ far_start, const int *__restrict__ far_n)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n_act = act_start[comp_count(P)];
    const int ntask = min((n_act + 63) >> 6, (int)(far.part_plane >> 6));      // (the partial sums' room: never short, see create.hip)
    const int nitem = ntask * ALLP_PARTS, nwg = (nitem + 3) >> 2;
    // (the launch is sized from the host's bound of the live count, the items from the device's own count.  The bound
    // covers the particles alive whatever is in flight -- StepLedger::alive_at_most, held to that by
    // tests/test_step_ledger_cpu.py -- so one round does; should a launch still be too small for them it takes several
    // rounds instead of leaving particles out: tests/test_gpu_state_swap.py ran these rounds on the library whose bound
    // an upload, a fill or a restore behind a step could leave too low)
    for (int b = blockIdx.x; b < nwg; b += gridDim.x) {
    // part-major: an XCD's contiguous eighth of the items is two parts -- an eighth of the far bodies, which then sit in its L2
    const int slot = xcd_contiguous(b, nwg) * 4 + wave;
    if (slot >= nitem) continue;
    const int part = slot / ntask, T = slot - part * ntask;
    const int r = T * 64 + lane;
    const bool valid = r < n_act;
    const int rr = valid ? r : T * 64;                      // (a lane past the end rides along on the task's first particle; nothing of it is stored)
    const int gi = dense_gi[rr], c = dense_cell[rr];
    const float4 me = snap4[gi];
    int i1, i2, i3;
    cell_coords(P, c, i1, i2, i3);
    const PairCtx ctx = {me.x, me.y, me.z, 0.f, 0, gi, false};
    const float eps2f = (float)P.eps2;
    const size_t plane = (size_t)far.plane;
    const int nblk = (P.num_cells_global + 63) >> 6;
    const int blk_lo = nblk * part / ALLP_PARTS, blk_hi = nblk * (part + 1) / ALLP_PARTS;
    float px = 0.f, py = 0.f, pz = 0.f;                     // the part's sum
    for (int blk = blk_lo; blk < blk_hi; blk++) {
        // the block's 64 cell ranges in one vector load, lane = cell (a scalar load per cell, and the body loads
        // behind it, were two dependent round trips for 64 bodies of work); with each cell's grid coordinates
        const int c2 = blk * 64 + lane;
        int f_nb = 0, f_cnt = 0, f_j = 0;
        if (c2 < P.num_cells_global) {
            int j1, j2, j3;
            global_coords(P, c2, j1, j2, j3);
            f_nb = far_start[c2];
            f_cnt = far_n ? far_n[c2] : min(far_start[c2 + 1] - f_nb, P.max_per_cell);
            f_j = pack_cell(j3, j1, j2);
        }
        for (int q0 = 0; q0 < 64; q0 += ALLP_CHUNK) {
            int n[ALLP_CHUNK], nb[ALLP_CHUNK];
            int total = 0, first = 0;
            bool adjacent = true, hit[ALLP_CHUNK], any_hit = false;
#pragma unroll
            for (int q = 0; q < ALLP_CHUNK; q++) {
                n[q] = __builtin_amdgcn_readlane(f_cnt, q0 + q);
                nb[q] = __builtin_amdgcn_readlane(f_nb, q0 + q);
                const int j = __builtin_amdgcn_readlane(f_j, q0 + q);
                if (n[q] > 0) {
                    if (total == 0) first = nb[q]; else adjacent = adjacent && nb[q] == first + total;
                    total += n[q];
                }
                hit[q] = n[q] > 0 && abs(packed_i3(j) - i3) <= 1 && abs(packed_i1(j) - i1) <= 1 && abs(packed_i2(j) - i2) <= 1;
                any_hit |= hit[q];
            }
            if (total == 0) continue;
            float ax = 0.f, ay = 0.f, az = 0.f;
            if (adjacent && !__any(any_hit)) {
                const float *sx = far_buf + first;
                acc_walk<MODE, NQ>(P, ctx, sx, sx + plane, sx + 2 * plane, sx + 3 * plane, total, eps2f, ax, ay, az);
            } else {
#pragma unroll
                for (int q = 0; q < ALLP_CHUNK; q++) {
                    if (n[q] == 0) continue;
                    const float kx = ax, ky = ay, kz = az;
                    const float *sx = far_buf + nb[q];
                    acc_walk<MODE, NQ>(P, ctx, sx, sx + plane, sx + 2 * plane, sx + 3 * plane, n[q], eps2f, ax, ay, az);
                    if (hit[q]) { ax = kx; ay = ky; az = kz; }      // a cell of this lane's own stencil: the cutoff pass has it
                }
            }
            px += ax; py += ay; pz += az;
        }
    }
    if (valid) far.part_acc[(size_t)part * far.part_plane + (size_t)r] = make_float4(px, py, pz, 0.f);
    }
}

// All-pairs: a particle's acceleration = (((stencil chain + part 0) + part 1) + ...) + part 15, the same
// association on one GPU and on any number of ranks.  One thread per particle that needs a force, in the dense order.
// NPARTS: the parts that were written, ALLP_PARTS of them unrolled, or 0: nparts of them (the pyramid's levels).
template <int NPARTS>
__global__ void k_allpairs_combine(DevParams P, const int *__restrict__ act_start, const int *__restrict__ dense_gi,
                                   const int *__restrict__ dense_cell, const FarCells far, int nparts, const ForceBuf force4)
{
    if (NPARTS) nparts = NPARTS;
    const int n = min(act_start[comp_count(P)], (int)far.part_plane);
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        const int gi = dense_gi[r], lc = dense_cell[r];
        float4 a = force4.get(P, lc, gi);                   // (flag 0, not a kid: it is on the active list)
#pragma unroll
        for (int p = 0; p < nparts; p++) {
            const float4 b = far.part_acc[(size_t)p * far.part_plane + (size_t)r];
            a.x += b.x; a.y += b.y; a.z += b.z;
        }
        force4.put(P, lc, gi, a);
    }
}

// The dense order of the pass (k_allp_prefix, k_allp_dense) and the sum of the parts (k_allpairs_combine) serve every far
// field that goes by (dense task, part) waves: the all-pairs one below and the monopoles' (farfield.hip), flat or as a pyramid.
// dense tasks: at most the particles alive (the host's bound; a slab also computes its neighbour's lent layers:
// every entry of the sorted order).  The kernels go by the device's own count.
int64_t far_dense_bound(const DevParams &P, const DeviceState &d, int64_t live_bound)
{
    return std::min<int64_t>(d.part_tasks, ((live_bound >= 0 && P.world == 1) ? live_bound : (int64_t)P.sorted_cap) / 64 + 2);
}

void launch_dense_order(hipStream_t st, const DevParams &P, const DeviceState &d)
{
    k_allp_prefix<<<1, 1024, 0, st>>>(P, d.active_count, d.act_start);
    k_allp_dense<<<(comp_count(P) + 3) / 4, 256, 0, st>>>(P, d.cell_start, d.active_list, d.active_count, d.act_start, d.dense_gi, d.dense_cell);
}

void launch_far_combine(hipStream_t st, const DevParams &P, const DeviceState &d, const FarCells &far, int nparts, int64_t dense_bound)
{
    const unsigned wgs = (unsigned)((dense_bound * 64 + 255) / 256);
    if (nparts == ALLP_PARTS) k_allpairs_combine<ALLP_PARTS><<<wgs, 256, 0, st>>>(P, d.act_start, d.dense_gi, d.dense_cell, far, nparts, force_buf(d));
    else k_allpairs_combine<0><<<wgs, 256, 0, st>>>(P, d.act_start, d.dense_gi, d.dense_cell, far, nparts, force_buf(d));
}

// What ran before is the stencil's chain (the two-pass pair stage: all-pairs contexts are created only with it, and only
// with lean arithmetic); now every other cell (k_allp_far) and the sum.  fast: the tolerance mode's arithmetic.
void launch_allpairs_far(hipStream_t st, const DevParams &P, const DeviceState &d, bool fast, int64_t live_bound)
{
    // where the far cells are found: pot_far_of (pot_walk.hpp)
    FarCells far;
    const PotFar src = pot_far_of(P, d, P.world > 1);
    far.plane = src.plane;
    far.part_acc = d.part_acc; far.part_plane = (unsigned long long)d.part_tasks * 64;
    const int64_t dense_bound = far_dense_bound(P, d, live_bound);
    launch_dense_order(st, P, d);
    const SnapSoa snap4{d.snap_soa, (size_t)P.sorted_cap};
    const unsigned far_wgs = (unsigned)((dense_bound * ALLP_PARTS + 3) / 4);
    if (fast) k_allp_far<2, 8><<<far_wgs, 256, 0, st>>>(P, snap4, d.act_start, d.dense_gi, d.dense_cell, far, src.buf, src.start, src.n);
    else k_allp_far<1, 8><<<far_wgs, 256, 0, st>>>(P, snap4, d.act_start, d.dense_gi, d.dense_cell, far, src.buf, src.start, src.n);
    launch_far_combine(st, P, d, far, ALLP_PARTS, dense_bound);
}

}  // namespace psamd
