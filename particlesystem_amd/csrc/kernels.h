// kernels.h -- host-visible launch wrappers of the kernel files.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/psamd.h"
#include "device_types.h"
#include "geometry.hpp"

namespace psamd {

// The on-stream services walk the owned slots in tiles of SLOT_TILE (slot_walk.hpp: export, potential, remove by box) and
// a caller's entries in tiles of ENTRY_TILE (multisplit.hpp: inject, remove by id)
constexpr int SLOT_TILE = 4096;
constexpr int ENTRY_TILE = 4096;
inline int slot_tiles(int slots_total) { return (slots_total + SLOT_TILE - 1) / SLOT_TILE; }
// what grows with a call's max_count (the host: grow_entry_scratch, services.hip)
struct EntryScratch {
    int2 *ent;        // [cap] per entry: its key -- the queue record, or a negative code of the service -- and its rank in the record
    int *tcount;      // [tiles * nrec] per tile and record: the count, then the exclusive prefix over the tiles
    int *tile_out;    // [tiles * words] the tile's side result (inject: its first entry outside the box; remove: three outcome counts)
    int64_t cap;      // entries there is room for
};

// psamd_export_live (export.hip): pass A leaves per tile its live count (DeviceState::exp_count) and these partials of the
// statistics (fp64 sums: mass, momentum x y z, kinetic energy, mass moment x y z, age; fp32 extrema: x, y, z, age)
constexpr int EXPORT_SUMS = 9;
struct __align__(16) ExportTile {
    double sum[EXPORT_SUMS];
    float lo[4], hi[4];
    int nonfinite, pad;
};
// where the chosen fields go (null: not wanted)
struct ExportFields {
    float4 *pos4, *vel4, *acc4;
    int *id, *cell;
};
// the count and statistics of psamd_download_live / psamd_live_stats_get (a caller of psamd_export_live may give its own)
struct ExportOut {
    int64_t count;
    psamd_live_stats stats;
};

// psamd_inject (inject.hip): the caller's arrays and the scratch
struct InjectArgs {
    const float4 *pos4, *vel4;
    const float *fert_age;
    int64_t max_count;
    const int64_t *count_dev;
    int *ids;
    psamd_inject_result *result;
};
struct InjectScratch {
    EntryScratch e;   // keys: the record, -1 not this rank's, -2 outside the box; tile_out: [tiles], INT_MAX: none outside
    int *removed;     // [nrec] slots the inject took from the record's queue
    int *hdr;         // [2] first entry outside the box, first queue failure
    psamd_inject_result *own;   // the context's own result record (psamd_inject_result_get)
};

// psamd_remove (remove.hip): by id the caller's entries, by box the owned slots.  All but `e` is sized at creation.
struct RemoveArgs {
    const int *ids;
    int64_t max_count;
    const int64_t *count_dev;
    int *outcome;
    psamd_remove_result *result;
};
struct RemoveScratch {
    EntryScratch e;   // keys: the record of a slot's first live occurrence, else -1 - outcome; tile_out: [tiles * 3] the outcomes 1, 2, 3
    int *claim;       // [slots] the lowest entry index that names the slot; INT_MAX between calls (a call restores what it claimed)
    int2 *ins;        // [nrec] the insert rule of a record the call adds to: offset of its first insert behind rloc, inserts the queue takes
    int *prefix;      // [slots + 1] by box: selected slots before this one in storage order
    int *tile_sel, *tile_live;   // [tiles of slots] by box: the tile's selected / live slots
    psamd_remove_result *own;    // the context's own result record (psamd_remove_result_get)
};

// psamd_update (update.hip): the caller's arrays and the scratch.  By id the claims are psamd_remove's claim words (the two
// services are ordered by the stream and each leaves the claims as it found them); code grows with a call's max_count (the
// host: grow_update_scratch, services.hip), the rest is sized at creation
constexpr int UPDATE_HDR_WORDS = 5;
struct UpdateArgs {
    uint32_t fields;
    const int *ids;
    const float4 *vel4;
    const float *w, *fert_age;
    int64_t max_count;
    const int64_t *count_dev;
    int *outcome;
    psamd_update_result *result;
};
struct UpdateScratch {
    int *code;        // [cap] by id, per entry: the storage index of its slot, or -1 - outcome
    int64_t cap;      // entries there is room for
    int *hdr;         // [UPDATE_HDR_WORDS] by id: the entries with the outcomes 0 .. 4
    int *tile_live;   // [tiles of slots] by export order: the tile's live slots
    psamd_update_result *own;    // the context's own result record (psamd_update_result_get)
};

// psamd_potential (potential.hip): the sorted order of the own cells in tiles of POT_TILE (tile t goes with tile t of the
// owned slots); per tile of the sorted order the partials of U (fp64), of phi's extrema and of the counts
constexpr int POT_TILE = SLOT_TILE;
struct __align__(16) PotTile {
    double u;
    float lo, hi;
    int listed, nonfinite;
    int pad[2];
};
// the context's own result record (psamd_potential_result_get), and the live count psamd_download_potential copies by
struct PotOut {
    psamd_potential_result result;
    int64_t live;
};

// psamd_probe (probe.hip): the caller's arrays and the scratch.  code / order grow with a call's max_count (the host:
// grow_probe_scratch, services.hip); the counters are sized at creation
constexpr int PROBE_HDR_WORDS = 4;
struct ProbeArgs {
    uint32_t fields;
    const float4 *pos4;
    int64_t max_count;
    const int64_t *count_dev;
    float4 *out4;
    int *outcome;
    psamd_probe_result *result;
};
struct ProbeScratch {
    int *code;        // [cap] per entry: its local cell, or -1 - outcome
    int *order;       // [cap] the served entries' indices, cell-major
    int64_t cap;      // entries there is room for
    int *counts;      // [n_local_cells + 1 + PROBE_HDR_WORDS] per cell: served entries, then their prefix; the header: nonfinite, served, outside, foreign
    psamd_probe_result *own;    // the context's own result record (psamd_probe_result_get)
};

// psamd_neighbours (neighbours.hip): what the caller gave, and the scratch.  All of the scratch is ONE allocation whose size
// depends on the container alone; the first call makes it (the host: neighbours_scratch, services.hip), contexts that never
// call the service hold none of it
struct NbrArgs {
    uint32_t flags;   // PSAMD_NEIGHBOURS_*
    float r2;         // RN(radius * radius)
    int *count, *nearest;       // [capacity] by export order (any may be null)
    float *nearest_d2;
    int64_t *offsets;           // [capacity + 1]
    int64_t capacity;
    int *list;                  // [list_capacity]
    int64_t list_capacity;
    psamd_neighbours_result *result;    // the caller's record (may be null)
};
struct __align__(16) NbrTile {  // what a tile of the sorted order saw of the queries
    long long pairs;  // the sum of their counts
    float d2_min;     // +inf: no neighbour
    int listed, max_count;
    int pad;
};
struct NbrOut {       // the context's own result record (psamd_neighbours_result_get), and the live count the host form copies by
    psamd_neighbours_result result;
    int64_t live;
};
struct NbrScratch {
    void *block;      // the one allocation; null: no call yet
    int *cnt_sorted, *who_sorted;   // [sorted_cap] per query, by sorted index: its count, its nearest neighbour's global slot id
    float *d2_sorted;               // ... and that pair's d2
    int *cnt_slot, *who_slot;       // [slots] the same by storage index; cnt -1: in no list of the frame
    float *d2_slot;
    int *index;       // [slots] storage index -> export index (-1: not live)
    long long *start; // [slots] storage index -> offsets[] of its entry (-1: past the capacity, or not live)
    NbrTile *tiles;   // [tiles of slots]
    int *tile_live;   // [tiles of slots] the tile's live slots
    long long *tile_sum;    // [tiles of slots] the counts of the tile's entries below the capacity
    NbrOut *own;
};
size_t neighbours_scratch_bytes(const DevParams &P);
void neighbours_scratch_carve(const DevParams &P, void *block, NbrScratch &s);

// psamd_groups (groups.hip): what the caller gave, and the scratch -- ONE allocation sized by the container alone, made by the
// first call (the host: groups_scratch, services.hip), like psamd_neighbours'
struct GrpArgs {
    uint32_t flags;   // PSAMD_GROUPS_*
    float r2;         // RN(radius * radius)
    int *group;       // [capacity] by export order (may be null)
    int64_t capacity;
    int *group_first, *group_size;      // [group_capacity] by group number (any may be null)
    int64_t group_capacity;
    psamd_groups_result *result;        // the caller's record (may be null)
};
struct __align__(16) GrpTile {  // what a tile of the owned slots holds
    int live, members, roots, singles;  // live slots; members; members that are their set's root; roots of a set of one
    int largest;      // the largest set rooted in the tile
    int pad[3];
};
struct GrpOut {       // the context's own result record (psamd_groups_result_get), and the live count the host form copies by
    psamd_groups_result result;
    int64_t live;
};
struct GrpScratch {
    void *block;      // the one allocation; null: no call yet
    int *parent;      // [slots] the union-find over storage indices: a word only ever falls (atomicMin), a root names itself
    int *member;      // [slots] 1: a listed particle of the own cells that is no kid
    int *root;        // [slots] the set's smallest storage index, once the hooking is over
    int *size;        // [slots] at a root: its set's members
    int *number;      // [slots] at a root: the dense group number
    int *index;       // [slots] storage index -> export index (-1: not live)
    GrpTile *tiles;   // [tiles of slots]
    unsigned long long *links;  // undirected links, each counted by its higher slot
    int *unfinished;  // unions that hit the step cap
    GrpOut *own;
};
size_t groups_scratch_bytes(const DevParams &P);
void groups_scratch_carve(const DevParams &P, void *block, GrpScratch &s);

// psamd_knn (knn.hip): what the caller gave, and the scratch -- ONE allocation sized by the container alone (never by k: the
// rows go straight to the caller's arrays), made by the first call (the host: knn_scratch, services.hip)
struct KnnArgs {
    uint32_t flags;   // PSAMD_KNN_*
    float r2;         // RN(radius * radius)
    int k;            // 1 .. PSAMD_KNN_MAX_K
    int *found;       // [capacity] by export order (may be null)
    int *who;         // [capacity * k] row-major (may be null)
    float *d2;        // [capacity * k] (may be null)
    int64_t capacity;
    psamd_knn_result *result;           // the caller's record (may be null)
};
struct __align__(16) KnnPart {  // what a task's wave saw of its queries
    int found, full, listed, pad;       // the sum of min(count, k); queries with count >= k; queries
    float dk_min, dk_max;               // the smallest / largest d2 of a k-th neighbour (+inf / -inf: no full query)
    float pad2[2];
};
struct KnnOut {       // the context's own result record (psamd_knn_result_get), and the live count the host form copies by
    psamd_knn_result result;
    int64_t live;
};
struct KnnScratch {
    void *block;      // the one allocation; null: no call yet
    int *index;       // [slots] storage index -> export index (-1: not live)
    int *tile_live;   // [tiles of slots] the tile's live slots
    KnnPart *parts;   // [own cells * slices] by task
    KnnOut *own;
};
size_t knn_scratch_bytes(const DevParams &P);
void knn_scratch_carve(const DevParams &P, void *block, KnnScratch &s);

// psamd_deposit (deposit.hip): the lattice, what the caller gave, and the scratch.  A task is (compute cell, block of at most
// 2 x 2 x 2 voxels of it): 1, 1 or 8 tasks a cell for refine 1, 2, 4; four tasks to a workgroup, whose partials are one entry
constexpr int DEPOSIT_WG_TASKS = 4;
inline int deposit_cell_tasks(int refine) { return refine == 4 ? 8 : 1; }
struct DepLattice {   // the lattice of refine k on a context's grid (the host: deposit_lattice, services.hip), psamd_sample's too
    int32_t refine;   // k: voxels per cell edge (1, 2 or 4)
    int32_t M;        // G * k voxels per axis
    float inv_h;      // (float)((double)k / cell_size)
    float off;        // (float)((G / 2) * k) - 0.5f
    float top;        // (float)(M - 1)
};
struct DepositArgs : DepLattice {
    float *out;       // [M^3] the lattice, voxel (n1, n2, n3) at (n3 * M + n1) * M + n2
    psamd_deposit_result *result;   // the caller's record (may be null)
};
struct DepositPart {  // what a workgroup's (up to) four tasks saw, merged in task order
    double mass;      // the tasks' voxel sums (fp64, before the rounding to float), in task and voxel order
    float vmax;       // the largest float written; -inf: none
    int bodies, skipped;    // of the tasks that count their own cell's list (a cell's first task)
    int pad;
};
struct DepositScratch {
    DepositPart *parts;     // [ceil(compute cells * 8 / 4)]: room for refine 4, sized at creation
    psamd_deposit_result *own;    // the context's own result record (psamd_deposit_result_get)
};

// psamd_sample (sample.hip): the caller's lattice on psamd_deposit's lattice, what else the caller gave, and the scratch.  By
// export order the tiles' live counts are psamd_update's (UpdateScratch::tile_live: the two services are ordered by the
// stream and each counts anew); all of it is sized at creation
constexpr int SAMPLE_HDR_WORDS = 3;
struct SampleArgs : DepLattice {
    uint32_t flags;   // PSAMD_SAMPLE_*
    float scale;
    const void *field;          // float[M^3] or float4[M^3], indexed as DepositArgs::out
    const float4 *pos4;         // null by export order
    int64_t max_count;
    const int64_t *count_dev;
    void *out;                  // float[max_count] or float4[max_count]
    int *outcome;
    psamd_sample_result *result;    // the caller's record, or the context's own
};
struct SampleScratch {
    int *hdr;         // [SAMPLE_HDR_WORDS] the entries served, outside, and of the served those with a word that is not finite
    psamd_sample_result *own;     // the context's own result record (psamd_sample_result_get)
};

// All-pairs force pass.  The cells beyond the stencil are found by GLOBAL cell in a snapshot buffer (the own
// one, or the all-gathered one of all ranks): x at buf[start], y, z, w_eff at multiples of `plane` behind.
// The stencil's chain comes from the ordinary (cutoff) force pass; the rest of a particle's sum is split into
// ALLP_PARTS partial sums, each by a wave of its own (or a lone rank of eight would have half a wave per SIMD
// walking the whole cloud): part p covers its share of the 64-cell blocks of the global cell order; partial sums
// land in part_acc[p * part_plane + r], r = the particle's place among those that need a force, and
// k_allpairs_combine adds them to the stencil's chain in part order (allpairs.hip, k_allp_far).
struct FarCells {
    unsigned long long plane = 0;
    float4 *part_acc = nullptr;
    unsigned long long part_plane = 0;
};
constexpr int ALLP_PARTS = 16;

// Every device allocation of a context.  SoA by slot unless noted.
struct DeviceState {
    // particle state, by slot (id == slot)
    float4 *pos4 = nullptr;       // x, y, z, w
    float4 *vel4 = nullptr;       // vx, vy, vz, age
    float4 *acc4 = nullptr;       // ax, ay, az, fertility_age
    int *cell = nullptr;          // -1 = free slot
    uint8_t *pflags = nullptr;    // bit0 is_parent
    uint32_t *tdata = nullptr;    // T_DATA_TYPE[container], 6 dwords each
    // free-slot queues (reference layout)
    QueueInfo *qinfo = nullptr;
    int *queue = nullptr;
    // per-frame grid
    int *cell_count = nullptr;    // [num_cells]   \ zeroed together
    int *chunk_count = nullptr;   // [num_chunks]  / by init_iframe
    uint8_t *chunk_skip = nullptr;   // [slots] 1: not in its chunk's (capped) list this frame; valid for the slots of over-cap chunks only
    int2 *chunk_segs = nullptr;      // [num_chunks * 27] (first slot, slots) of the segments a chunk's particles live in, in slot order
    FrameScalars *fs = nullptr;
    FrameScalars *fs_host = nullptr;  // the host's TWO pinned records as the device sees them (the step's number picks one; written by the queue-census kernels)
    StepState *st = nullptr;          // the step's number and the scalar records' sequence number, device-resident
    int *cell_start = nullptr;    // [num_cells+1]
    int *cursor = nullptr;        // [num_cells]
    int *task_start = nullptr;    // [num_cells+1] prefix of 64-particle slices per cell
    int *task_list = nullptr;     // [num_cells * slices] non-empty (cell, slice) tasks, cell-major
    // two-pass pair stage (lean modes): collision flags first, forces only where they are used
    int *halo_count = nullptr;    // [num_cells] collision candidates listed by the neighbours (zeroed with the frame)
    float *halo_f = nullptr;      // [3][num_cells * HALO_CAP] x, y, z of those candidates
    int *halo_id = nullptr;       // [num_cells * HALO_CAP] their slot ids
    int *snap_cid = nullptr;      // [container] sorted order: slot id, or -1 for a body that can never collide
    int *active_list = nullptr;   // [container] per cell (at cell_start[c]): sorted indices of the particles that need a force (written by k_collide_cell)
    int *active_count = nullptr;  // [num_cells] zeroed with the frame
    int *task_list2 = nullptr;    // [num_cells * slices]
    // balanced force pass: every wave walks the same number of bodies; a task may be cut at a stencil-cell boundary
    int *task_cost = nullptr;     // [local cells] bodies in the cell's stencil = what one task of the cell walks
    int *ctask_start = nullptr;   // [computed cells + 1] first entry of task_list2 of the j-th computed cell
    long long *cost_start = nullptr;  // [computed cells + 1] cost of all tasks before the j-th computed cell
    long long *wave_pos = nullptr; // [waves + 1] where every wave slot of the balanced pass starts: task index << 32 | cost already walked inside the task
    int *task_ready = nullptr;    // [num_cells * slices] hand-off flags, zeroed with the frame
    int4 *merged_tasks = nullptr; // [num_cells] cells whose leftover slices share one wave (-1: unused)
    int4 *pack_stage = nullptr;   // [num_cells, whole windows] the same, window by window as k_pack_windows leaves them (pack_fit.hpp)
    int *pack_count = nullptr;    // [windows] packs of every window of 64 computed cells
    int *pack_base = nullptr;     // [windows] the first pack of every window (k_plan_force, where its LDS does not hold them)
    // the merged tasks run beside k_pairs on a stream of their own (fork / join by events)
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int *sorted_id = nullptr;     // [container] cell-major, id ascending inside a cell
    float *snap_soa = nullptr;    // [4][sorted_cap] sorted order: x, y, z, w_eff as four arrays (what the pair walk streams)
    float *snap_age = nullptr;    // [container] sorted order
    float4 *force4 = nullptr;     // [sorted_cap] sorted order: (ax, ay, az, flag) of the lent region's particles; the hand-off mailbox of the force pass
    int *cell_order = nullptr;    // [n_own_cells] the own (local) cells by (chunk, segment type, cell in the segment): cells that share a segment's slots side by side
    uint8_t *flag_slot = nullptr; // [slots] by slot: the step's collision flag of the own cells' particles (their new acceleration goes into acc4.xyz: ForceBuf, kernels_common.hpp)
    CellInfo *celltab = nullptr;  // [num_cells]
    // lifecycle
    uint64_t *op_keys = nullptr, *op_keys_sorted = nullptr;
    int *op_args = nullptr, *op_args_sorted = nullptr;
    int ops_cap = 0;
    int *rec_count = nullptr;     // [queue_infos] zeroed with the frame
    int *rec_start = nullptr;     // [queue_infos + 1]
    int *rec_cursor = nullptr;    // [queue_infos]
    MoveRec *moves = nullptr;
    int moves_cap = 0;
    float4 *stage = nullptr;      // 3 float4 per move
    XferRec *xfer_out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // slab mode: records leaving for the rank below / above, two ranks below / above (inside the messages)
    int *status_out = nullptr;    // slab mode: [0] cell-overflow kills this frame, [1] error bits, [2] live, [16..] the killed slot ids
    // all-pairs across ranks: the gathered snapshot blocks (inside the context's message buffer) and their index by global cell
    const int *allg_in = nullptr;
    int *gstart = nullptr, *gn = nullptr;
    float4 *part_acc = nullptr;   // all-pairs: [ALLP_PARTS][part_tasks * 64] partial sums of the far pass's (dense task, part) waves
    int part_tasks = 0;
    int *act_start = nullptr;     // all-pairs: [num_cells + 1] particles that need a force in the pass's cells before its j-th
    int *dense_gi = nullptr;      // all-pairs: [container] sorted index of the r-th particle that needs a force (cell order)
    int *dense_cell = nullptr;    // all-pairs: [container] its cell
    // far monopoles (PSAMD_FLAG_FAR_MONOPOLE; part_acc .. dense_cell above are this pass's too): per cell of the box,
    // padded with zeros to whole blocks of 64 cells, the planes X, Y, Z, M and the cell's packed grid coordinates
    float *cell_mom = nullptr;    // [4][mom_cap]; with quadrupoles (PSAMD_FLAG_FAR_QUADRUPOLE) [10][mom_cap]: Cxx, Cyy, Czz, Cxy, Cxz, Cyz behind
    int *cell_mom_j = nullptr;    // [mom_cap] (i3 << 20) | (i1 << 10) | i2
    int mom_cap = 0;
    // the levels of those planes (mom_cap == lev.off[lev.n]): one, the cell grid, on a flat context; on the pyramid
    // (PSAMD_FLAG_FAR_PYRAMID) every level, level 0 first, so the cells' moments are where the far monopoles have them, and
    // the fp64 sums S, Sx, Sy, Sz the levels add up
    FarLevels lev;
    double *lev_sum = nullptr;    // [4][mom_cap]; with quadrupoles [10][mom_cap]: the raw Sxx, Syy, Szz, Sxy, Sxz, Syz behind
    // a far slab (PSAMD_FLAG_FAR_SLAB, world > 1; allg_in above is its gathered cell sums): (first global cell, cells) of
    // every rank's state layers, and lev_sum also on the flat method
    int *far_plan = nullptr;      // [world][2]
    DevCounters *ctr = nullptr;
    // psamd_export_live: per tile of SLOT_TILE owned slots, the live count and the statistics' partials; the context's own result record
    int *exp_count = nullptr;
    ExportTile *exp_tiles = nullptr;
    ExportOut *exp_out = nullptr;
    // psamd_potential: phi by sorted index and by slot, per tile the partials and the live count, the context's own result record
    float *pot_sorted = nullptr;
    float *pot_slot = nullptr;
    PotTile *pot_tiles = nullptr;
    int *pot_count = nullptr;
    PotOut *pot_out = nullptr;
    unsigned long long *trace = nullptr;  // 3 words per pair-kernel wave slot (diagnostic builds only)
};

hipError_t launch_unpack_aos(hipStream_t st, const DevParams &P, const void *aos, int first, int count, float half_box,
                             const DeviceState &d);
hipError_t launch_pack_aos(hipStream_t st, const DevParams &P, void *aos, int first, int count, const DeviceState &d);
hipError_t launch_place(hipStream_t st, const DevParams &P, int n, const int *ids, const float4 *p, const float4 *v, const float4 *a,
                        const int *cells, const DeviceState &d);
hipError_t launch_fill_int(hipStream_t st, int *p, int v, size_t n);
hipError_t launch_restore(hipStream_t st, int n, const void *s_pos, const void *s_vel, const void *s_acc,
                          const void *s_cell, const void *s_flags, const void *s_queue, const void *s_qinfo, int qinfo_words,
                          int step, const DeviceState &d);
hipError_t launch_validate_eps(hipStream_t st, uint32_t lo_bits, uint32_t hi_bits, double eps2, float eps2f,
                               unsigned long long *out);
hipError_t launch_selftest_math(hipStream_t st, uint32_t lo_bits, uint32_t hi_bits, unsigned long long *out24);
hipError_t launch_init_tdata(hipStream_t st, const DevParams &P, const DeviceState &d);
// ev (optional) = 5 events recorded before hist, scan, scatter, sort and after sort.  tdata_rows: also write the reference's T_DATA rows (a mirror for
// psamd_download_tdata; nothing in the step reads them).  big_cells: launch the instance for cells of more than 1024 ids
// (a hint: without it such a cell is ranked through global memory by the ordinary instance).
hipError_t launch_build_grid(hipStream_t st, const DevParams &P, const DeviceState &d, hipEvent_t *ev, bool tdata_rows, bool big_cells);
// psamd_download_force4: entries [first, first + count) of the sorted order, gathered from where the records live
hipError_t launch_force_gather(hipStream_t st, const DevParams &P, const DeviceState &d, void *out, int first, int count);
// tasks_hint: about how many force tasks the pass will have (sizes the balanced force pass)
// pass: 0 or 1, which of a frame's (up to two) passes of the pair stage this is
// live_bound: at most so many particles are alive (< 0: unknown); sizes the all-pairs far pass's launch
hipError_t launch_pairs(hipStream_t st, const DevParams &P, const DeviceState &d, hipEvent_t ev_force, int64_t tasks_hint, int pass, int64_t live_bound);
// what shapes launch_pairs' launches for this hint, as a number below 2^24 (the key of a captured graph)
uint64_t launch_pairs_shape(const DevParams &P, int64_t tasks_hint);
// launch_pairs' launches outside force.hip, in the order it makes them (their errors are launch_pairs' to collect):
// the collision flags (collide.hip), the plan of the balanced force pass (plan.hip: nw wave slots, merge: with packs),
// the far field of the all-pairs forces and its sum (allpairs.hip; fast: the tolerance mode's arithmetic), or the far
// monopoles and theirs (farfield.hip)
void launch_collide(hipStream_t st, const DevParams &P, const DeviceState &d);
void launch_plan_force(hipStream_t st, const DevParams &P, const DeviceState &d, int nw, bool merge, int pass);
void launch_allpairs_far(hipStream_t st, const DevParams &P, const DeviceState &d, bool fast, int64_t live_bound);
// ... and what allpairs.hip shares with the far monopoles: the host's bound of the dense tasks, the dense order of the
// particles that need a force (act_start, dense_gi, dense_cell), the sum of the nparts parts that were written onto the
// stencil's chain in part order
int64_t far_dense_bound(const DevParams &P, const DeviceState &d, int64_t live_bound);
void launch_dense_order(hipStream_t st, const DevParams &P, const DeviceState &d);
void launch_far_combine(hipStream_t st, const DevParams &P, const DeviceState &d, const FarCells &far, int nparts, int64_t dense_bound);
// the moments of a far-monopole context's frame, of the cells or of every level of the pyramid (farfield.hip): the pair
// stage's, and the far forms of psamd_potential and psamd_probe, which may run before it
void launch_far_moments(hipStream_t st, const DevParams &P, const DeviceState &d);
// the far field of a far-monopole context, flat or as a pyramid (farfield.hip): the moments, then a particle's far set -- every
// cell beyond its stencil as one body, or per level the cells under the neighbours of its parent that are not its own cell's
// neighbours (the top level: all that are not) -- and the parts' sum, the pyramid's top level first
void launch_far_field(hipStream_t st, const DevParams &P, const DeviceState &d, bool fast, int64_t live_bound);
hipError_t launch_apply(hipStream_t st, const DevParams &P, const SegLayout &S, const DeviceState &d);
hipError_t launch_frame_reset(hipStream_t st, const DeviceState &d, size_t frame_ints, int status_table);   // also clears the status record's header and census table
// The step's tail behind k_apply: census of the queue operations (+ relocation phase 1), bucketing (the step's scalars go
// out to the host's pinned record), replay + commit + the next frame's init_iframe.  live_hint sizes grid-stride
// launches and nothing else; cap0 (2048 / 4096 / 8192) picks the replay instance -- lists longer than it are sorted in
// global memory by the same workgroup.  frame_ints / status_table: what the next frame's reset zeroes.
hipError_t launch_lifecycle(hipStream_t st, const DevParams &P, const DeviceState &d, int nrec, int64_t live_hint, int cap0,
                            size_t frame_ints, int status_table);
// slab exchange (messages are int arrays with a 16-word header, see kernels.hip)
// the snapshots for the rank below (k = 0) / above (k = 1), both in one pair of launches; also closes the status record
hipError_t launch_pack_halos(hipStream_t st, const DevParams &P, const DeviceState &d, const int c0[2], const int ncell[2],
                             int *const msg[2], int *const pack_off[2]);
hipError_t launch_unpack_halos(hipStream_t st, const DevParams &P, const DeviceState &d, int ncell_below, const int *msg_below,
                               int *off_below, int ncell_above, const int *msg_above, int *off_above);
hipError_t launch_pack_force(hipStream_t st, const DevParams &P, const DeviceState &d, int *msg, int cap_bodies);
hipError_t launch_outbox_close(hipStream_t st, const DevParams &P, const DeviceState &d, int64_t live_hint, int *const msgs[5]);
hipError_t launch_inbox_merge(hipStream_t st, const DevParams &P, const DeviceState &d, const int *const msgs[5]);
hipError_t launch_allg_pack(hipStream_t st, const DevParams &P, const DeviceState &d, int *msg);
hipError_t launch_allg_index(hipStream_t st, const DevParams &P, const DeviceState &d);
// a far slab's message (farfield.hip): the fp64 sums of the own cells from the snapshot, straight into the block that is
// all-gathered (slab_build); then, from the gathered blocks of all ranks, level 0 of the box and the levels above it
// (slab_pairs) -- after which the moments are those of one context
hipError_t launch_far_own_sums(hipStream_t st, const DevParams &P, const DeviceState &d, int *msg);
hipError_t launch_far_gathered(hipStream_t st, const DevParams &P, const DeviceState &d);
// the chunk lists' capacity rule over all ranks' status records (start of the pair stage)
hipError_t launch_chunk_census(hipStream_t st, const DevParams &P, const DeviceState &d, const int *status_all);
// status records of all ranks (error bits, cell-overflow kills, the transfer messages' next capacity) + the force records of the lent-out layers (force_msg, may be null)
hipError_t launch_status_merge(hipStream_t st, const DevParams &P, const DeviceState &d, const int *status_all,
                               int force_j0, const int *force_msg, const int *pack_off);

// psamd_export_live: pass A over every owned slot, then pass B (the chosen fields of the first `capacity` live particles in
// slot order; workgroup 0 writes the count and the statistics)
hipError_t launch_export_live(hipStream_t st, const DevParams &P, const DeviceState &d, const ExportFields &out,
                              int64_t capacity, int64_t *count_out, psamd_live_stats *stats_out);

// psamd_potential: phi of every particle in the own cells' lists (k_pot_pairs), U and the extrema in a fixed tree, phi of the
// first `capacity` live particles in slot order (phi null or capacity 0: the result alone); result_dev may be null.
// flags: the spec's, validated.  PSAMD_POTENTIAL_FAR (far-monopole contexts only): the moments first, then the cell's far set
// behind the stencil; with PSAMD_POTENTIAL_QUADRUPOLE (quadrupole contexts only) every member's quadrupole term too
hipError_t launch_potential(hipStream_t st, const DevParams &P, const DeviceState &d, float *phi, int64_t capacity,
                            psamd_potential_result *result_dev, uint32_t flags);

// psamd_probe (max_count > 0): locate + count, the cells' prefix, the cell-major order, the pair pass (one probe to a lane), the
// result record
hipError_t launch_probe(hipStream_t st, const DevParams &P, const DeviceState &d, const ProbeArgs &a, const ProbeScratch &s);

// psamd_neighbours: the count walk over the own cells' (cell, slice) tasks, the three launches on the slot walk (to slot
// order and the tiles' partials; the slot -> export index table and the tiles' sums; the record, the export-order arrays and
// offsets), then -- a.list given -- the same walk again, storing the names
hipError_t launch_neighbours(hipStream_t st, const DevParams &P, const DeviceState &d, const NbrArgs &a, const NbrScratch &s);

// psamd_groups: the sets' start, the hooking walk over psamd_neighbours' tasks, then three launches on the slot walk (the roots
// and the sizes; the group numbers, the slot -> export index table and the two tables; the record and group[])
hipError_t launch_groups(hipStream_t st, const DevParams &P, const DeviceState &d, const GrpArgs &a, const GrpScratch &s);

// psamd_knn: two launches on the slot walk (the tiles' live counts; the slot -> export index table and the default rows), the
// walk over psamd_neighbours' tasks that keeps each query's best k and stores its row, then the record over the tasks' partials
hipError_t launch_knn(hipStream_t st, const DevParams &P, const DeviceState &d, const KnnArgs &a, const KnnScratch &s);

// psamd_deposit: the gather over the compute cells' tasks, then the result record (mass, vmax and the counts over the
// workgroups' partials in task order)
hipError_t launch_deposit(hipStream_t st, const DevParams &P, const DeviceState &d, const DepositArgs &a, const DepositScratch &s);

// psamd_inject: locate + rank, the records' prefix, the first queue failure, the placement, the commit of the queues and
// the result record (max_count > 0)
hipError_t launch_inject(hipStream_t st, const DevParams &P, const SegLayout &S, const DeviceState &d, int nrec, const InjectArgs &a,
                         const InjectScratch &s);

// psamd_remove by id (max_count > 0): the first occurrences' claims, the entries' ranks, the records' commit and the result
// record, the placement; by box: the tiles' counts, the slots' prefix, the commit, the placement (every owned slot)
hipError_t launch_remove_ids(hipStream_t st, const DevParams &P, const SegLayout &S, const DeviceState &d, int nrec, const RemoveArgs &a,
                             const RemoveScratch &s);
hipError_t launch_remove_box(hipStream_t st, const DevParams &P, const SegLayout &S, const DeviceState &d, int nrec, const float lo[3],
                             const float hi[3], bool outside, psamd_remove_result *result, const RemoveScratch &s);

// psamd_update by id (max_count > 0; claim: psamd_remove's claim words): the first
// occurrences' claims, the writes and outcomes, the result record; by export order: the tiles' live counts, then the writes,
// the outcomes and the result record
hipError_t launch_update_ids(hipStream_t st, const DevParams &P, const DeviceState &d, const UpdateArgs &a, const UpdateScratch &s,
                             int *claim);
hipError_t launch_update_order(hipStream_t st, const DevParams &P, const DeviceState &d, const UpdateArgs &a, const UpdateScratch &s);
// ... the first pass of the order form on its own: per tile of SLOT_TILE owned slots the live slots (psamd_sample's too)
hipError_t launch_live_tiles(hipStream_t st, const DevParams &P, const DeviceState &d, int *tile_live);

// psamd_sample (max_count > 0): the three counters zeroed, one pass over the entries (the points form) or the tiles' live
// counts and one pass over the owned slots (by export order; tile_live: psamd_update's), the result record
hipError_t launch_sample(hipStream_t st, const DevParams &P, const DeviceState &d, const SampleArgs &a, const SampleScratch &s,
                         int *tile_live);

}  // namespace psamd
