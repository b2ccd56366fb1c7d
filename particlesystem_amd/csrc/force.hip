// force.hip -- calc_forces' second neighbour loop: the forces over the 27-cell stencil (ps.cpp:1247-1263), and
// launch_pairs, the pair stage's launches in order
#include "pair_math.hpp"
#include "tile_walk.hpp"

namespace psamd {

// One wave = 64 consecutive particles of one cell (four independent waves per workgroup).
// Neighbour cells are visited in the reference's stencil order, their bodies in list
// order, and every lane adds each body to its own particle's sum: each particle sees
// exactly the reference's sequence of fp32 additions (ps.cpp:1247-1259).
// MODE 0: exact with the compiler's correctly rounded sqrt/divide (any EPS2);
//      1: exact with pair_math.hpp's short sqrt/reciprocal, NQ pairs per slow-branch test;
//      2: fast math (FMA + v_rsq), not bit-exact.
//
// Modes 1 and 2 never stage neighbour data at all.  It is the same for all 64 lanes, the
// ranges are wave-uniform, so the loads are scalar loads (s_load_dwordx8 from the SoA
// snapshot, straight out of L2 into SGPRs) and the packed fp32 instructions take the SGPR
// pairs as operands: no LDS, no vector registers for the bodies.  (An LDS tile read with
// ds_read_b128 by four waves per CU kept the LDS pipe ~70 % busy -- 16 cycles per wave
// read, scripts/microbench/lds_groups.hip -- and cost 4 % more time.)
// (Round 4 tried a third way -- every row of 16 lanes holds 16 bodies in VGPRs and the arithmetic takes them through
// DPP, `v_sub_f32_dpp rx, tile_x, xi row_newbcast:j`: no LDS, no scalar loads, the compiler fuses every broadcast.
// Bit-identical and 9-17 % slower everywhere: a DPP-modified v_sub / v_mul issues at half rate on gfx950.
// profiles/r4_ab_dpp_walk.txt, commit 2592be9.)
// Mode 0, the fallback for softening lengths outside the lean range, streams 64-body
// tiles through 1 KiB of LDS per wave.  No s_barrier: a wave only ever touches its own
// tile, and a wave's LDS operations complete in issue order, so a compiler-level fence
// is all the ordering needed.

#ifdef PSAMD_WAVE_TRACE   // diagnostic build only: when and where did this wave run
#define PS_TRACE_BEGIN() const unsigned long long trace_t0 = __builtin_amdgcn_s_memrealtime()
#define PS_TRACE_END() do { if ((threadIdx.x & 63) == 0) { \
        unsigned long long *t_ = trace + (size_t)3 * (blockIdx.x * 4 + (threadIdx.x >> 6)); \
        t_[0] = trace_t0; t_[1] = __builtin_amdgcn_s_memrealtime(); \
        t_[2] = ((unsigned long long)(__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 0xf) << 32)   /* XCC_ID */ \
                | __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4); } } while (0)               /* HW_ID */
#else
#define PS_TRACE_BEGIN() do {} while (0)
#define PS_TRACE_END() do {} while (0)
#endif

// Stencil steps [k0, k1) of a task.  The sums of the steps before k0 > 0 come from the wave that walked them (hand-off
// through `ready`); a walk that stops before step 27 publishes its sums instead of finishing the particle.  Its callers:
//   k_pairs, the one-pass stage: whole tasks (k0 = 0, k1 = 27, no hand-off, no pacing) cut from the cells' own lists
//     (active_list == nullptr); the walk settles the collision flags on its way.  MODE 0 walks through `tile`.
//   k_pairs_balanced, the two-pass stage (MODE 1, 2): pieces of tasks cut from the lists of the particles that need a
//     force, the flags known already (SETTLED: nothing tracks distances for them), paced; no tile.
// (MODE 0 stays a branch of this function: as a function of its own k_pairs<0, 4> took 50 VGPRs instead of 49.)
template <int MODE, int NQ, bool SETTLED>
__device__ __forceinline__ void pairs_task(const DevParams &P, const int *__restrict__ cell_start,
                                           const SnapSoa snap4, const float *__restrict__ snap_soa,
                                           const float *__restrict__ snap_age, const int *__restrict__ sorted_id,
                                           const ForceBuf force4, int task,
                                           float4 *tile, unsigned long long *trace,
                                           const int *__restrict__ active_list, const int *__restrict__ active_count,
                                           int k0, int k1, int *ready, FrameScalars *fs, WavePace *pace)
{
    PS_TRACE_BEGIN();
    const int c = task / P.slices, slice = task - c * P.slices;
    const int base = cell_start[c];
    // two-pass mode: the slice is cut from the cell's list of particles that need a force
    const int cnt = active_list ? active_count[c] : min(cell_start[c + 1] - base, P.max_per_cell);
    const int first = slice * 64;
    if (first >= cnt) return;
    const int nvalid = min(64, cnt - first);
    const int lane = threadIdx.x & 63;
    const bool valid = lane < nvalid;
    const int gi = active_list ? active_list[base + first + (valid ? lane : 0)] : base + first + (valid ? lane : 0);
    const float4 me = snap4[gi];
    const float age_i = snap_age[gi];
    const int id_i = sorted_id[gi];
    const bool dead = age_i > P.life_thr;                      // ps.cpp:1183
    const bool kid = age_i < P.kid_thr;
    const bool scan = SETTLED ? false : (valid && !dead && !kid && !active_list);   // two-pass mode: flags are settled already

    int i1, i2, i3;
    cell_coords(P, c, i1, i2, i3);
    float ax = 0.f, ay = 0.f, az = 0.f;
    int flag = 0;
    const float eps2f = (float)P.eps2;

    // Lane k (< 27) looks up neighbour cell k of the stencil once: its range in the
    // sorted order, or an empty range if it lies outside the grid.
    int my_nb = 0, my_cnt = 0;
    if (lane < 27) {
        const int nc = local_cell(P, i3 + c_stencil[lane][2], i1 + c_stencil[lane][1], i2 + c_stencil[lane][0]);
        if (nc >= 0) {
            my_nb = cell_start[nc];
            my_cnt = min(cell_start[nc + 1] - my_nb, P.max_per_cell);
        }
    }
    if (MODE != 0) {
        const PairCtx ctx = {me.x, me.y, me.z, age_i, id_i, gi, scan};
        const size_t cap = (size_t)P.sorted_cap;
        if (k0 > 0 && !handoff_consume(force4 + gi, ax, ay, az, flag, valid, ready, k0)) {
            if (lane == 0) atomicOr(&fs->error, ERR_HANDOFF_TIMEOUT);
        }
        // The bodies [nb, nb + n) of one cell, from four planes of a snapshot (wave-uniform pointers: scalar loads).
        auto walk_cell = [&](const float *__restrict__ sx, const float *__restrict__ sy, const float *__restrict__ sz,
                             const float *__restrict__ sw, int nb, int n) {
            float dmin = 3.0e38f;
            int jj = 0;
            // NQ bodies per group.  (Fetching the next group between the distance stage and
            // the rest -- scalar loads return out of order, so it cannot go out any earlier --
            // was measured 3 % slower for the exact arithmetic on a full GPU and no faster
            // on a 1/8 share.)
            for (; jj + NQ <= n; jj += NQ) {
                v2f qx[NQ / 2], qy[NQ / 2], qz[NQ / 2], qw[NQ / 2];
                load_group<NQ>(sx, sy, sz, sw, jj, qx, qy, qz, qw);
                // (The compiler lets the masses' load sink to its use, behind the reciprocal square roots; pinned up
                // here with the coordinates' loads -- four in one batch -- the pass took the same time, 2.13 ms.)
                if (MODE == 1)
                    pairsN_exact_lean<NQ>(P, ctx, qx, qy, qz, qw, nb + jj, snap_age, sorted_id, ax, ay, az, flag);
                else
                    dmin = fminf(dmin, pairsN_fast<NQ>(ctx, qx, qy, qz, qw, eps2f, ax, ay, az));
            }
            for (; jj < n; jj++) {
                const float4 q = make_float4(sx[jj], sy[jj], sz[jj], sw[jj]);
                if (MODE == 1)
                    pair1_exact_lean(P, ctx, q, nb + jj, snap_age, sorted_id, ax, ay, az, flag);
                else
                    dmin = fminf(dmin, pair_fast(me.x, me.y, me.z, q, eps2f, ax, ay, az));
            }
            // fast math, rare: someone in this cell is within the (widened) collision gate of
            // one of my lanes; the exact rule is then evaluated on unfused distances
            const float gate_soft = (P.coll_d2_gate + eps2f) * 1.0001f;
            if (MODE == 2 && __any(scan && !(dmin > gate_soft))) {
                if (scan && !(dmin > gate_soft)) {
                    for (int j = 0; j < n; j++) {
                        const float rx = sx[j] - me.x, ry = sy[j] - me.y, rz = sz[j] - me.z;
                        const float d2 = rx * rx + ry * ry + rz * rz;
                        if (!(d2 > P.coll_d2_gate) && nb + j != gi)
                            flag = max(flag, collide_exact(P, d2, age_i, id_i, snap_age[nb + j], sorted_id[nb + j]));
                    }
                }
            }
        };
        // the stencil, in the reference's order
        for (int k = k0; k < k1; k++) {
            const int nb = __builtin_amdgcn_readlane(my_nb, k), n = __builtin_amdgcn_readlane(my_cnt, k);
            const float *sx = snap_soa + nb;
            walk_cell(sx, sx + cap, sx + 2 * cap, sx + 3 * cap, nb, n);
            if (pace) pace->step();
        }
    } else {
        // Generic exact mode: tiles of 64 snapshot entries, in stencil order then list order.
        // The next tile's global load is issued before the current tile is consumed.  The lean
        // modes let a particle meet itself (r = 0 adds +0, exactly nothing) because
        // 1/sqrt(eps2^3) is finite on the range they are allowed on; this one also serves
        // softening lengths where it is not, so it skips the self pair explicitly, as the
        // reference does by id (ps.cpp:1258), and a kid neighbour too (app_common.cu:240: ai
        // comes back unchanged; its zeroed mass times an infinite 1/r^3 would be a NaN).
        int k = 0, t0 = 0;
        int nb = __shfl(my_nb, 0), ncnt = __shfl(my_cnt, 0);
        while (ncnt == 0 && ++k < 27) { nb = __shfl(my_nb, k); ncnt = __shfl(my_cnt, k); }
        bool have = k < 27;
        float4 pre = make_float4(0.f, 0.f, 0.f, 0.f);
        if (have && lane < min(64, ncnt)) pre = snap4[nb + lane];
        while (have) {
            const int c_nb = nb, c_t0 = t0, n = min(64, ncnt - t0);
            PS_WAVE_SYNC();                           // previous tile fully consumed
            if (lane < n) tile[lane] = pre;
            PS_WAVE_SYNC();
            t0 += 64;                                 // advance to the next non-empty tile
            if (t0 >= ncnt) {
                t0 = 0; ncnt = 0;
                while (ncnt == 0 && ++k < 27) { nb = __shfl(my_nb, k); ncnt = __shfl(my_cnt, k); }
            }
            have = k < 27;
            // issued after the fences (they drain outstanding loads), consumed a tile later
            if (have && lane < min(64, ncnt - t0)) pre = snap4[nb + t0 + lane];
            float dmin = 3.0e38f, dsum = 0.0f;          // (dsum: a distance that is not a number passes the collision test; fminf drops it)
#pragma unroll 4
            for (int jj = 0; jj < n; jj++) {
                if (c_nb + c_t0 + jj == gi) continue;
                const float4 q = tile[jj];
                if (q.w == 0.0f) {                     // kid (or massless) neighbour: no force term, still a distance
                    const float rx = q.x - me.x, ry = q.y - me.y, rz = q.z - me.z;
                    const float d2 = rx * rx + ry * ry + rz * rz;
                    dmin = fminf(dmin, d2); dsum += d2;
                    continue;
                }
                const float d2 = pair_exact(me.x, me.y, me.z, q, P.eps2, ax, ay, az);
                dmin = fminf(dmin, d2); dsum += d2;
            }
            // rare: someone in this tile is within the collision gate of one of my lanes
            const bool close = scan && (!(dmin > P.coll_d2_gate) || dsum != dsum);
            if (__any(close)) {
                if (close) {
                    for (int jj = 0; jj < n; jj++) {
                        const float4 q = tile[jj];
                        const float rx = q.x - me.x, ry = q.y - me.y, rz = q.z - me.z;
                        const float d2 = rx * rx + ry * ry + rz * rz;
                        const int gj = c_nb + c_t0 + jj;
                        if (!(d2 > P.coll_d2_gate) && gj != gi)
                            flag = max(flag, collide_exact(P, d2, age_i, id_i, snap_age[gj], sorted_id[gj]));
                    }
                }
            }
        }
    }
    if (MODE != 0 && k1 < STENCIL) {             // not the end of the walk: hand the sums on
        handoff_publish(force4 + gi, ax, ay, az, flag, valid, ready, k1);
        PS_TRACE_END();
        return;
    }
    if (dead) flag = 2;
    if (kid) { ax = 0.f; ay = 0.f; az = 0.f; }   // every term is skipped for a kid (app_common.cu:240)
    if (MODE != 0 && !SETTLED) {
        // one-pass lean stage: a particle whose own position is not a number met itself and the kids (stencil_adults;
        // the two-pass stage settles this in k_collide_cell, the generic mode skips both explicitly)
        const bool lost = valid && !kid && !finite3(me.x, me.y, me.z);
        if (__any(lost)) {
            const int adults = stencil_adults(P, i1, i2, i3, cell_start, snap_age);       // (all lanes: the count is a wave's work)
            if (lost && adults <= 1) { ax = 0.f; ay = 0.f; az = 0.f; }
        }
    }
    if (valid) force4.put_id(P, c, gi, id_i, make_float4(ax, ay, az, __int_as_float(flag)));
    PS_TRACE_END();
}

template <int MODE, int NQ>
__global__ __launch_bounds__(256) void k_pairs(DevParams P, const int *__restrict__ cell_start,
                                               const SnapSoa snap4,
                                               const float *__restrict__ snap_soa,
                                               const float *__restrict__ snap_age,
                                               const int *__restrict__ sorted_id,
                                               const int *__restrict__ task_list,
                                               const ForceBuf force4,
                                               FrameScalars *fs, unsigned long long *trace,
                                               const int *__restrict__ active_list, const int *__restrict__ active_count)
{
    // (active_list, active_count: null at both launches -- the one-pass stage cuts its tasks from the cells' own lists.
    // They stay kernel parameters for the register allocation alone: with the nulls spelled out in here the lean
    // instances came out with 87 / 66 VGPRs instead of 79 / 62, five waves per SIMD instead of six for the exact one.)
    // Workgroups of four INDEPENDENT waves (no workgroup barrier anywhere): the hardware
    // deals a workgroup's waves over the four SIMDs of its CU and workgroups over the
    // CUs, which keeps even a small share (a few waves per CU) evenly spread.
    __shared__ float4 tiles[MODE == 0 ? 4 : 1][MODE == 0 ? 64 : 1];   // mode 0 only
    const int wave = threadIdx.x >> 6;
    // The work list holds only non-empty (cell, slice) tasks, cell-major.  Workgroups are dealt
    // round-robin over the eight XCDs (b and b + 8 share an L2), so workgroup b takes its four
    // tasks from XCD (b & 7)'s contiguous eighth of the list: neighbouring cells' snapshots then
    // sit in that XCD's L2.
    // (Eighths of equal WORK instead of equal length -- the outer planes of the grid have
    // fewer neighbours, so the two XCDs holding them go idle for the last sixth of the
    // launch -- were tried: the XCDs then finish together, yet the launch was only 1 %
    // shorter and the extra prefix sum cost k_scan 10 us.)
    const int ntask = active_list ? fs->n_tasks2 : fs->n_tasks;
    const int nwg = (ntask + 3) >> 2;
    if ((int)blockIdx.x >= nwg) return;
    const int slot = xcd_contiguous(blockIdx.x, nwg) * 4 + wave;
    if (slot >= ntask) return;
    pairs_task<MODE, NQ, false>(P, cell_start, snap4, snap_soa, snap_age, sorted_id, force4,
                                task_list[slot], tiles[MODE == 0 ? wave : 0], trace, active_list, active_count, 0, STENCIL, nullptr, fs, nullptr);
}

// The force pass, balanced: `nw` waves (all resident), wave slot s walks the (task, stencil step)
// units from wave_pos[s] up to wave_pos[s + 1] -- the same number of bodies for every wave
// (k_split_tasks).  Most of a wave's share is whole tasks; the task its share ends in is started
// FIRST (steps 0 .. k-1, sums published), then the whole tasks, and LAST the task its share
// begins in is finished from the sums the previous wave slot published at the very start of its
// own work -- so nobody waits in practice, and a particle's sum is still one serial chain of
// fp32 additions in the reference's order.  A share that lies inside one task (few tasks, many
// waves) is one middle piece: consume, walk, publish.
// Wave slots are dealt XCD by XCD like the tasks of k_pairs; k_split_tasks starts every XCD's
// run at a whole task, so the wave that continues a task runs in a workgroup that was
// dispatched no later (block b - 8) or is the same workgroup.
// WALK 0: scalar-load walk (pairs_task) for the ordinary tasks, and the packs of partial slices in
//         workgroups of their own at the head of the launch;
//      1: tile walk (pairs_task_tile) for the ordinary tasks, no packs (few waves per SIMD).
// nmb (WALK 0, a multiple of 8 so that the XCD dealing is undisturbed): the first nmb workgroups of the
// launch serve the merged packs of partly filled slices instead (merged_pack_task) -- dispatched first,
// their waves are the oldest on their SIMDs and are served first, which is what lets these long,
// stall-prone waves finish well inside the pass.  (As a kernel of their own on a second stream they
// needed a head start to get that: forked at the same moment as the balanced pass they ended with it,
// and the stage took 0.1 ms longer.)
template <int MODE, int NQ, int WALK>
__global__ __launch_bounds__(256, WALK == 0 ? BALANCED_WAVES : 2) void k_pairs_balanced(DevParams P, const int *__restrict__ cell_start,
                                                        const SnapSoa snap4,
                                                        const float *__restrict__ snap_soa,
                                                        const float *__restrict__ snap_age,
                                                        const int *__restrict__ sorted_id,
                                                        const int *__restrict__ task_list,
                                                        const ForceBuf force4,
                                                        FrameScalars *fs, unsigned long long *trace,
                                                        const int *__restrict__ active_list, const int *__restrict__ active_count,
                                                        const long long *__restrict__ wave_pos, int *__restrict__ task_ready,
                                                        const int4 *__restrict__ merged_tasks, int nmb, StepState *st, int pass)
{
    __shared__ __attribute__((aligned(16))) float tiles[4][4 * MERGE_TILE];   // up to four 1-KiB tiles per wave (a pack's four groups)
    const int wave = threadIdx.x >> 6;
#ifdef PSAMD_WAVE_TRACE   // (diagnostic build: the wave's whole life, first instruction to last piece -- overwrites what its pieces noted)
    const unsigned long long wave_t0 = __builtin_amdgcn_s_memrealtime();
    struct WholeWave {
        unsigned long long *trace; unsigned long long t0;
        __device__ ~WholeWave() { if ((threadIdx.x & 63) == 0) { unsigned long long *t_ = trace + (size_t)3 * (blockIdx.x * 4 + (threadIdx.x >> 6)); t_[0] = t0; t_[1] = __builtin_amdgcn_s_memrealtime(); } }
    } whole_wave{trace, wave_t0};
#endif
    if (WALK == 0 && (int)blockIdx.x < nmb) {
        // The packs of partly filled slices, dealt round-robin to the 4 * nmb pack waves: a pack wave takes every
        // (4 * nmb)-th pack, one after the other, and paces itself over all of them -- so the launch holds the number of
        // pack workgroups that the packs' share of the WORK asks for, whatever their number (N = 2^22 in 24^3 cells has
        // 6 900 packs: one workgroup per four of them would be the whole GPU).
        const int first = blockIdx.x * 4 + wave, stride = nmb * 4, npack = fs->n_merged;
        if (first < npack) {
            WavePace pace;                       // a pack is 27 steps of (up to) four cells' stencils
            const int ticks = st->pairs_ticks[pass];
            pace.t0 = st->pairs_t0[pass];
            pace.per_tick = ticks > 0 ? 1.0f / (float)ticks : 0.f;
            pace.per_unit = 1.0f / (float)(STENCIL * ((npack - first + stride - 1) / stride));
            for (int pack = first; pack < npack; pack += stride)     // (4 bodies per group: the 8-wide form costs this kernel its sixth wave per SIMD)
                merged_pack_task<MODE, 4>(P, cell_start, snap4, active_list, active_count, merged_tasks, force4, pack, tiles[wave], pace);
        }
        return;
    }
    const int slot = xcd_contiguous((int)blockIdx.x - nmb, (int)gridDim.x - nmb) * 4 + wave;
    const long long pos_b = wave_pos[slot], pos_e = wave_pos[slot + 1];
    if (pos_e <= pos_b) return;                              // (positions order like units: task-major, cost inside the task)
    const int ub = resolve_unit(P, pos_b, cell_start, task_list), ue = resolve_unit(P, pos_e, cell_start, task_list);
    if (ue <= ub) return;
    WavePace pace;
    if (WALK == 0) {
        const int ticks = st->pairs_ticks[pass];
        pace.t0 = st->pairs_t0[pass];
        pace.per_tick = ticks > 0 ? 1.0f / (float)ticks : 0.f;
        pace.per_unit = 1.0f / (float)(ue - ub);
    }
    struct PassEnd {        // the pass's end, for the next one's clock: the latest wave's last instruction
        StepState *st; int pass; bool on;
        __device__ ~PassEnd() { if (on && (threadIdx.x & 63) == 0) atomicMax(&st->pairs_end[pass], (unsigned long long)__builtin_amdgcn_s_memrealtime()); }
    } pass_end{st, pass, WALK == 0};
    const int tb = ub / STENCIL, lb = ub - tb * STENCIL;            // first unit: task tb, step lb
    const int tl = (ue - 1) / STENCIL, le = ue - tl * STENCIL;      // last task tl, its steps [.., le)
    // one call site, so one copy of the walk: the pieces in the order they are done
    const bool single = tb == tl;
    const int has_head = (!single && le < STENCIL) ? 1 : 0, has_tail = (!single && lb > 0) ? 1 : 0;
    const int first_whole = tb + has_tail, last_whole = tl + (has_head ? 0 : 1);      // tasks walked whole: [first, last)
    const int nwhole = single ? 0 : last_whole - first_whole;
    const int pieces = single ? 1 : has_head + nwhole + has_tail;
    for (int i = 0; i < pieces; i++) {
        int t, k0 = 0, k1 = STENCIL;
        if (single) { t = tb; k0 = lb; k1 = le; }
        else if (has_head && i == 0) { t = tl; k1 = le; }                 // the head of the last task first: publish early
        else if (i - has_head < nwhole) t = first_whole + (i - has_head);
        else { t = tb; k0 = lb; }                                         // the tail of the first task last: its head was published long ago
        const int nord = fs->n_tasks2;
        if (WALK == 1) {
            // task t: an ordinary (cell, slice) task, or -- past them -- merged pack t - n_tasks2.  (The plan lists no
            // packs for a tile-walk pass, so the second form is never taken.  Without it the compiler allocates the walk
            // differently -- 238 VGPRs instead of 256 -- and the pass took 1 % longer on an eighth of the N = 2^20 cloud.)
            TileGroups G;
            if (t < nord) {
                const int task = task_list[t], c = task / P.slices, slice = task - c * P.slices;
                G.ng = 1; G.cell[0] = c; G.first[0] = slice * 64; G.count[0] = min(64, active_count[c] - slice * 64);
                G.cell[1] = G.cell[2] = G.cell[3] = c; G.first[1] = G.first[2] = G.first[3] = 0; G.count[1] = G.count[2] = G.count[3] = 0;
            } else {
                const int4 pk = merged_tasks[t - nord];
                const int cells[4] = {pk.x, pk.y, pk.z, pk.w};
                G.ng = 0;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const bool on = cells[q] >= 0;
                    G.cell[q] = on ? cells[q] : pk.x;
                    G.first[q] = on ? (active_count[cells[q]] & ~63) : 0;
                    G.count[q] = on ? (active_count[cells[q]] & 63) : 0;
                    if (on) G.ng = q + 1;
                }
            }
            if (t < nord) pairs_task_tile<MODE, NQ, 1, false>(P, cell_start, snap4, force4, G, tiles[wave], active_list, k0, k1, task_ready + t, fs);
            else pairs_task_tile<MODE, NQ, 4, false>(P, cell_start, snap4, force4, G, tiles[wave], active_list, k0, k1, task_ready + t, fs);
        } else
            pairs_task<MODE, NQ, true>(P, cell_start, snap4, snap_soa, snap_age, sorted_id, force4, task_list[t], nullptr, trace,
                                       active_list, active_count, k0, k1, task_ready + t, fs, &pace);      // (per_tick == 0: no pacing)
    }
}

// How one pass of the pair stage is launched, from the hint of its task count: everything that shapes the
// launches and is not read from device memory by the kernels themselves (what a captured graph is keyed by).
struct PairShape {
    bool two;                // two-pass stage: collision flags first, then the balanced force pass
    bool tile;               // ... with the tile walk and no packs (WALK 1); else the scalar walk and the packs (WALK 0)
    int nw;                  // wave slots of the balanced force pass
    int nmb;                 // workgroups of the same launch, ahead of them, that serve the packs of partly filled slices (WALK 0)
};

constexpr double PACK_COST = 1.4;      // a pack's walk in ordinary tasks: four lane groups, each with its own LDS tile

static PairShape pair_shape(const DevParams &P, bool lean, int64_t hint)
{
    const int64_t tasks_hint = hint & 0xffffffffll, packs_hint = hint >> 32;      // (step.hip, pairs_hint)
    PairShape s{};
    s.two = lean && P.two_pass;
    if (!s.two) return s;
    // Balanced pass: a fixed number of waves, all resident, each walking the same number of
    // bodies.  At least four per SIMD when there are that many tasks (fewer cannot cover their
    // scalar-load latency: 1024 / 2048 / 4096 / 6144 waves took 3.73 / 2.54 / 2.27 / 2.29 ms on
    // the N = 2^20 cloud), but not more waves than tasks (a task cut in three or more pieces is
    // a chain of waves that wait for each other).
    s.nw = 1024 * (int)std::min<int64_t>(BALANCED_WAVES, std::max<int64_t>(1, tasks_hint / 1024));
    // Few waves per SIMD (a slab of a multi-GPU run): the scalar-load walk cannot cover its own load latency,
    // bodies come through LDS tiles fetched a tile ahead instead, and the partly filled last slices stay
    // ordinary tasks.  A pack wave is long and stalls on its tile loads; a share this small has too little other
    // work to cover that (an eighth of the N = 2^20 cloud, tile walk: no packs 0.58 ms, packs 0.60).
    s.tile = s.nw <= 2048;
    if (s.tile) return s;
    // The packs of partly filled last slices: persistent workgroups at the head of the launch, sized by the packs'
    // share of the work, their waves paced (a slab of two: pair stage 1.32 -> 1.12 ms against packs in the task list).
    // They hold residency slots for about half of the launch: with a wave slot for every resident wave besides, the
    // workgroups dispatched last could only start when a pack ended (wave trace, round 4: a quarter of the balanced
    // waves started 0.6-0.9 ms into a 2.3-ms launch).  So the balanced part gets as many wave slots as the packs leave
    // free: everything is resident from the start.  How many pack workgroups: the packs' share of the pass's work, in
    // workgroups of the resident set; a pack wave takes several packs one after the other.  Without a hint (a
    // context's first step) a quarter.
    const int resident = s.nw / 4;                     // workgroups the launch keeps resident
    if (s.nw >= 4096) {
        const double pw = PACK_COST * (double)packs_hint, tw = (double)std::max<int64_t>(tasks_hint - packs_hint, 1);
        const double share = packs_hint > 0 ? pw / (pw + tw) : 0.25;
        int wgs = ((int)(resident * share + 0.5) + 7) & ~7;
        wgs = std::max(8, std::min(wgs, resident / 2));
        if (packs_hint > 0) wgs = std::min(wgs, (int)(((packs_hint + 3) / 4 + 7) & ~7));      // (a pack wave with no pack is a wasted slot)
        s.nmb = wgs;
        s.nw = (s.nw - 4 * wgs) & ~255;
    } else
        s.nmb = (int)std::min<int64_t>(((packs_hint > 0 ? (packs_hint + 3) / 4 : resident / 4) + 7) & ~7, resident);
    return s;
}

uint64_t launch_pairs_shape(const DevParams &P, int64_t tasks_hint)
{
    const PairShape s = pair_shape(P, P.lean_math != 0, tasks_hint);
    return (uint64_t)(s.nw / 32) | (s.tile ? 1ull << 10 : 0) | (s.two ? 1ull << 11 : 0) | ((uint64_t)(s.nmb / 8) << 12);
}

template <int MODE, int NQ>
static hipError_t launch_pairs_mode(hipStream_t st, const DevParams &P, const DeviceState &d, hipEvent_t ev_force, int64_t tasks_hint, int pass, int64_t live_bound)
{
    const int ncomp = comp_count(P);
    if (ncomp <= 0) return hipSuccess;
    const ForceBuf fbuf = force_buf(d);
    const int tasks = ncomp * P.slices;
    const SnapSoa snap4{d.snap_soa, (size_t)P.sorted_cap};
    // softening lengths outside the lean range (MODE 0): the one-pass stage with the generic exact arithmetic, nothing else
    // (a context with all-pairs forces is created only with lean arithmetic)
    const PairShape shape = pair_shape(P, MODE != 0, tasks_hint);
    if (shape.two) {
        // collision flags and the per-cell lists of the particles that need a force, then the plan of the force pass
        launch_collide(st, P, d);
        launch_plan_force(st, P, d, shape.nw, !shape.tile, pass);
    }
    if (ev_force) (void)hipEventRecord(ev_force, st);      // timing: the force pass proper starts here
    if constexpr (MODE != 0) {
        if (shape.two) {
            // the hand-off flags are indexed by task number, which starts at 0 in every pass of a frame:
            // each pass has its own block of them (both zeroed with the frame)
            int *task_ready = d.task_ready + (size_t)pass * P.n_local_cells * P.slices;
            // the packs of partly filled slices: the first nmb workgroups of the same launch (scalar walk only)
            const int nmb = shape.nmb;
#define PS_BALANCED(W, Q) k_pairs_balanced<MODE, Q, W><<<nmb + shape.nw / 4, 256, 0, st>>>(P, d.cell_start, snap4, d.snap_soa, \
        d.snap_age, d.sorted_id, d.task_list2, fbuf, d.fs, d.trace, d.active_list, d.active_count, d.wave_pos, task_ready, d.merged_tasks, nmb, d.st, pass)
            // The tile walk -- a wave with its SIMD (almost) to itself -- takes 16 bodies per group: every group costs such a
            // wave two branches on a vector compare and the tail of three chains of dependent additions, all of it exposed;
            // half as many groups: -5 % on the pair stage of an eighth of the N = 2^20 cloud, -6 % in the tolerance mode (profiles/r4_ab_tile_nq.txt).
            // (The next group's distances between a group's scale factors and its additions, in one basic block: 9 % SLOWER.)
            // (The same in the scalar walk where a SIMD holds four waves -- N = 2^22 on eight ranks -- gave 1 %: not kept.)
            if (shape.tile) PS_BALANCED(1, 16); else PS_BALANCED(0, NQ);
#undef PS_BALANCED
            if (P.flags & PSAMD_FLAG_ALL_PAIRS) launch_allpairs_far(st, P, d, MODE == 2, live_bound);
            else if (P.flags & (PSAMD_FLAG_FAR_MONOPOLE | PSAMD_FLAG_FAR_PYRAMID)) launch_far_field(st, P, d, MODE == 2, live_bound);
            return hipGetLastError();
        }
    }
    k_pairs<MODE, NQ><<<(tasks + 3) / 4, 256, 0, st>>>(P, d.cell_start, snap4, d.snap_soa, d.snap_age, d.sorted_id, d.task_list, fbuf, d.fs, d.trace, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_pairs(hipStream_t st, const DevParams &P, const DeviceState &d, hipEvent_t ev_force, int64_t tasks_hint, int pass, int64_t live_bound)
{
    if (!P.lean_math) return launch_pairs_mode<0, 4>(st, P, d, ev_force, tasks_hint, pass, live_bound);
    // fast math shares the lean modes' validity range (finite 1/sqrt(eps2^3))
    if (P.flags & PSAMD_FLAG_FAST_MATH) return launch_pairs_mode<2, 8>(st, P, d, ev_force, tasks_hint, pass, live_bound);
    // 8 pairs per slow-branch test: measured 3 % (full GPU) to 5 % (a 1/8 share) faster than 4
    return launch_pairs_mode<1, 8>(st, P, d, ev_force, tasks_hint, pass, live_bound);
}

}  // namespace psamd
