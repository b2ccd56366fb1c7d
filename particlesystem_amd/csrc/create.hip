// create.hip -- making and describing a context: psamd_create as a sequence of named parts, psamd_destroy,
// psamd_describe and the getters of sizes, configuration and slab plan.
#include <cmath>
#include <new>

#include "context.hpp"

const char *psamd::status_text(int s)
{
    switch (s) {
    case PSAMD_OK: return "ok";
    case PSAMD_ERR_INVALID_ARG: return "invalid argument";
    case PSAMD_ERR_NO_DEVICE: return "no usable HIP device (the HIP path is the only path)";
    case PSAMD_ERR_HIP: return "HIP runtime error";
    case PSAMD_ERR_OUT_OF_MEMORY: return "out of device memory";
    case PSAMD_ERR_OUTSIDE_BOX: return "particle location outside box";
    case PSAMD_ERR_QUEUE_EMPTY: return "overflow: reserved space of the segment is full";
    case PSAMD_ERR_CELL_OVERFLOW: return "cell or queue-op capacity exceeded on device";
    case PSAMD_ERR_STATE: return "stage called out of order";
    case PSAMD_ERR_UNSUPPORTED: return "unsupported";
    }
    return "unknown status";
}

extern "C" {

int psamd_abi_version(void) { return PSAMD_ABI_VERSION; }
const char *psamd_status_string(int status) { return status_text(status); }
const char *psamd_last_error(const psamd_ctx *c) { return c ? c->err.c_str() : "null context"; }

int psamd_default_config(psamd_config *cfg)
{
    if (!cfg) return PSAMD_ERR_INVALID_ARG;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->max_particles_num = 1024 * 1024;  // common.h:12
    cfg->x_factor = 2;                     // common.h:13
    cfg->chunk_factor = 4;                 // common.h:29
    cfg->chunk_dim = 4;                    // common.h:30
    cfg->cell_size = 5.0;                  // common.h:52
    cfg->eps2 = 0.2;                       // common.h:53
    cfg->collision_radius = 0.4;           // common.h:54
    cfg->particle_weight = 60.0;           // common.h:55
    cfg->dt = 0.05;                        // common.h:69
    cfg->max_v = 10.0;                     // common.h:66
    cfg->explosion_speed = 3.0;            // common.h:67
    cfg->life_steps = 300.0;               // common.h:58
    cfg->device = 0;
    cfg->flags = 0;
    cfg->seed = 1;                         // RAND_SEED, common.h:56
    cfg->rank = 0;
    cfg->world = 1;
    cfg->drag = 0.0;
    cfg->force_sign = 1.0;
    return PSAMD_OK;
}

// What a far pass by (dense task, part) waves needs, the all-pairs one and the monopoles': the partial sums -- one float4 per
// (part, particle that needs a force), dense, 64 to a task; every entry of the sorted order could be one -- and the dense order.
static int alloc_dense_parts(psamd_ctx *c, size_t SC, size_t LC)
{
    DeviceState &d = c->d;
    d.part_tasks = (int)(SC / 64 + 1);
    PS_HIP(c, dev_alloc(c, &d.part_acc, (size_t)ALLP_PARTS * d.part_tasks * 64));
    PS_HIP(c, dev_alloc(c, &d.act_start, LC + 1));
    PS_HIP(c, dev_alloc(c, &d.dense_gi, SC));
    PS_HIP(c, dev_alloc(c, &d.dense_cell, SC));
    return PSAMD_OK;
}

// The step's device arrays.  The SEQUENCE of the HIP calls here is load-bearing, the copies and fills between the
// allocations included (the runtime allocates on their first use): with the three fills and the chunk_segs copy moved
// behind the last allocation the all-pairs step measured 0.15-0.17 % slower, with the same kernels (see also ctask_start).
static int alloc_step_arrays(psamd_ctx *c, const std::vector<int> &far_plan)
{
    const Geometry &g = c->geo; const DevParams &P = c->P; DeviceState &d = c->d;
    const size_t C = (size_t)P.slots_total;          // owned slots
    const size_t SC = (size_t)P.sorted_cap + 64;     // sorted-order arrays (+ slack: scalar loads fetch whole groups)
    const size_t LC = (size_t)P.n_local_cells;
    int *frame = nullptr;
    PS_HIP(c, dev_alloc(c, &d.pos4, C));
    PS_HIP(c, dev_alloc(c, &d.vel4, C));
    PS_HIP(c, dev_alloc(c, &d.acc4, C));
    PS_HIP(c, dev_alloc(c, &d.cell, C));
    PS_HIP(c, dev_alloc(c, &d.pflags, C));
    PS_HIP(c, dev_alloc(c, &d.tdata, 6 * C));
    PS_HIP(c, dev_alloc(c, &d.qinfo, (size_t)g.queue_infos));
    PS_HIP(c, dev_alloc(c, &d.queue, C));
    PS_HIP(c, dev_alloc(c, &frame, c->frame_ints));
    d.cell_count = frame; d.chunk_count = frame + LC; d.rec_count = d.chunk_count + g.num_chunks;
    d.rec_cursor = d.rec_count + g.queue_infos;
    d.halo_count = d.rec_cursor + g.queue_infos;
    d.active_count = d.halo_count + LC;
    d.task_ready = d.active_count + LC;
    PS_HIP(c, dev_alloc(c, &d.halo_f, (size_t)3 * LC * HALO_CAP + 64));   // + slack: scalar loads fetch whole groups
    PS_HIP(c, dev_alloc(c, &d.halo_id, LC * HALO_CAP + 64));
    PS_HIP(c, dev_alloc(c, &d.active_list, SC));
    PS_HIP(c, dev_alloc(c, &d.snap_cid, SC));
    PS_HIP(c, dev_alloc(c, &d.task_list2, LC * P.slices));
    PS_HIP(c, dev_alloc(c, &d.merged_tasks, LC));
    PS_HIP(c, dev_alloc(c, &d.task_cost, LC));
    // (LC + 1 entries are used.  At LC + 1 the later allocations move and the all-pairs step measured 0.1-0.2 % slower,
    // with the same kernels.)
    PS_HIP(c, dev_alloc(c, &d.ctask_start, 2 * LC + 2));
    PS_HIP(c, dev_alloc(c, &d.cost_start, 2 * LC + 2));
    PS_HIP(c, dev_alloc(c, &d.wave_pos, (size_t)MAX_PAIR_WAVES + 1));
    PS_HIP(c, dev_alloc(c, &d.rec_start, (size_t)g.queue_infos + 1));
    PS_HIP(c, dev_alloc(c, &d.fs, 1));
    PS_HIP(c, dev_alloc(c, &d.st, 1));
    PS_HIP(c, hipMemsetAsync(d.st, 0, sizeof(StepState), c->stream));
    PS_HIP(c, dev_alloc(c, &d.cell_start, LC + 1));
    PS_HIP(c, dev_alloc(c, &d.cursor, LC));
    PS_HIP(c, dev_alloc(c, &d.task_start, LC + 1));
    PS_HIP(c, dev_alloc(c, &d.task_list, LC * P.slices));
    PS_HIP(c, dev_alloc(c, &d.sorted_id, SC));
    PS_HIP(c, dev_alloc(c, &d.flag_slot, C));
    PS_HIP(c, dev_alloc(c, &d.snap_soa, 4 * (size_t)P.sorted_cap + 64));
    PS_HIP(c, dev_alloc(c, &d.snap_age, SC));
    PS_HIP(c, dev_alloc(c, &d.force4, SC));
    PS_HIP(c, dev_alloc(c, &d.celltab, (size_t)g.num_cells));
    if (P.flags & PSAMD_FLAG_ALL_PAIRS) PS_TRY(alloc_dense_parts(c, SC, LC));
    PS_HIP(c, dev_alloc(c, &d.chunk_skip, C));               // the chunk lists' capacity rule (chunk_cap_block)
    PS_HIP(c, dev_alloc(c, &d.chunk_segs, (size_t)g.num_chunks * 27));
    {
        std::vector<int2> segs((size_t)g.num_chunks * 27);
        for (int ch = 0; ch < g.num_chunks; ch++) {
            Pair pk[27];
            g.chunk_segments(ch, pk);
            for (int j = 0; j < 27; j++) {
                const int k = seg_index(pk[j].c);
                segs[(size_t)ch * 27 + j] = make_int2(g.seg_base[k] + pk[j].p * g.seg_size_t[k], g.seg_size_t[k]);
            }
            // slot order (set_pkg_segments lists them so already; the walk must not depend on it)
            std::sort(segs.begin() + (size_t)ch * 27, segs.begin() + (size_t)ch * 27 + 27, [](const int2 &a, const int2 &b) { return a.x < b.x; });
        }
        PS_HIP(c, hipMemcpy(d.chunk_segs, segs.data(), segs.size() * sizeof(int2), hipMemcpyHostToDevice));
    }
    PS_HIP(c, dev_alloc(c, &d.op_keys, (size_t)d.ops_cap));
    PS_HIP(c, dev_alloc(c, &d.op_keys_sorted, (size_t)d.ops_cap));
    PS_HIP(c, dev_alloc(c, &d.op_args, (size_t)d.ops_cap));
    PS_HIP(c, dev_alloc(c, &d.op_args_sorted, (size_t)d.ops_cap));
    // the host polls these records (wait_scalars): coherent mapping whatever HIP_HOST_COHERENT says, and zeroed --
    // hipHostMalloc does not promise zeroed pages, and a recycled page whose seq word happened to hold the number
    // the first step waits for would be taken for that step's scalars
    PS_HIP(c, hipHostMalloc((void **)&c->h_fs, 2 * sizeof(FrameScalars), hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(c->h_fs, 0, 2 * sizeof(FrameScalars));
    PS_HIP(c, hipHostGetDevicePointer((void **)&c->d.fs_host, c->h_fs, 0));
    PS_HIP(c, dev_alloc(c, &d.moves, (size_t)d.moves_cap));
    PS_HIP(c, dev_alloc(c, &d.stage, 3 * (size_t)d.moves_cap));
    PS_HIP(c, dev_alloc(c, &d.ctr, (size_t)COUNTER_COPIES));
    PS_HIP(c, dev_alloc(c, &d.exp_count, (size_t)slot_tiles(P.slots_total)));     // psamd_export_live's scratch
    PS_HIP(c, dev_alloc(c, &d.exp_tiles, (size_t)slot_tiles(P.slots_total)));
    PS_HIP(c, dev_alloc(c, &d.exp_out, 1));
    PS_HIP(c, dev_alloc(c, &d.pot_sorted, SC));                                      // psamd_potential's scratch and result record
    PS_HIP(c, dev_alloc(c, &d.pot_slot, C));
    PS_HIP(c, dev_alloc(c, &d.pot_tiles, (size_t)slot_tiles(P.slots_total)));
    PS_HIP(c, dev_alloc(c, &d.pot_count, (size_t)slot_tiles(P.slots_total)));
    PS_HIP(c, dev_alloc(c, &d.pot_out, 1));
    PS_HIP(c, hipMemsetAsync(d.pot_out, 0, sizeof(PotOut), c->stream));
    PS_HIP(c, dev_alloc(c, &c->inj.removed, (size_t)g.queue_infos));    // psamd_inject's fixed scratch and result record
    PS_HIP(c, dev_alloc(c, &c->inj.hdr, 2));
    PS_HIP(c, dev_alloc(c, &c->inj.own, 1));
    PS_HIP(c, hipMemsetAsync(c->inj.own, 0, sizeof(psamd_inject_result), c->stream));
    PS_HIP(c, dev_alloc(c, &c->rem.claim, C));                          // psamd_remove's fixed scratch and result record
    PS_HIP(c, dev_alloc(c, &c->rem.ins, (size_t)g.queue_infos));
    PS_HIP(c, dev_alloc(c, &c->rem.prefix, C + 1));
    PS_HIP(c, dev_alloc(c, &c->rem.tile_sel, (size_t)slot_tiles(P.slots_total)));
    PS_HIP(c, dev_alloc(c, &c->rem.tile_live, (size_t)slot_tiles(P.slots_total)));
    PS_HIP(c, dev_alloc(c, &c->rem.own, 1));
    PS_HIP(c, hipMemsetAsync(c->rem.own, 0, sizeof(psamd_remove_result), c->stream));
    // psamd_probe's fixed scratch and result record: a counter per local cell (a rank serves the cells it computes, lent-in
    // layers included, so the own cells alone would not do), one word more, the header
    PS_HIP(c, dev_alloc(c, &c->prb.counts, LC + 1 + PROBE_HDR_WORDS));
    PS_HIP(c, dev_alloc(c, &c->prb.own, 1));
    PS_HIP(c, hipMemsetAsync(c->prb.own, 0, sizeof(psamd_probe_result), c->stream));
    PS_HIP(c, dev_alloc(c, &d.trace, 3 * (LC * P.slices + 4)));
    PS_HIP(c, hipMemsetAsync(d.trace, 0, 3 * (LC * P.slices + 4) * sizeof(unsigned long long), c->stream));
    // the packs of the leftovers by window (pack_fit.hpp); last, so that nothing older moves
    PS_HIP(c, dev_alloc(c, &d.pack_stage, LC + 64));
    PS_HIP(c, dev_alloc(c, &d.pack_count, LC / 64 + 1));
    PS_HIP(c, dev_alloc(c, &d.pack_base, LC / 64 + 1));
    if (P.flags & (PSAMD_FLAG_FAR_MONOPOLE | PSAMD_FLAG_FAR_PYRAMID)) {
        // the far field of monopoles, behind everything a context without the flags allocates: the partial sums and the dense
        // order (a pyramid's level is a part: at most FAR_MAX_LEVELS of the ALLP_PARTS planes are used), and the moments --
        // four planes and the packed coordinates of every level (flat: the cell grid alone), each level padded to whole
        // blocks of 64 cells; the padding stays zero (the kernels write the cells of a level); under the pyramid's flag only,
        // the fp64 sums the levels are added up from.  With quadrupoles (PSAMD_FLAG_FAR_QUADRUPOLE) six planes more of each:
        // the central second moments behind X, Y, Z, M and the raw ones behind S, Sx, Sy, Sz
        const bool pyramid = (P.flags & PSAMD_FLAG_FAR_PYRAMID) != 0;
        const size_t planes = (P.flags & PSAMD_FLAG_FAR_QUADRUPOLE) ? 10 : 4;
        static_assert(FAR_MAX_LEVELS <= ALLP_PARTS, "a level's sum goes into one of the partial-sum planes");
        PS_TRY(alloc_dense_parts(c, SC, LC));
        d.mom_cap = d.lev.off[d.lev.n];
        PS_HIP(c, dev_alloc(c, &d.cell_mom, planes * (size_t)d.mom_cap + 64));     // + slack: scalar loads fetch whole groups
        PS_HIP(c, dev_alloc(c, &d.cell_mom_j, (size_t)d.mom_cap));
        // (a slab keeps the sums on the flat method too: level 0 is scattered there from the gathered blocks)
        const bool sums = pyramid || P.world > 1;
        if (sums) PS_HIP(c, dev_alloc(c, &d.lev_sum, planes * (size_t)d.mom_cap));
        PS_HIP(c, hipMemsetAsync(d.cell_mom, 0, (planes * (size_t)d.mom_cap + 64) * sizeof(float), c->stream));
        PS_HIP(c, hipMemsetAsync(d.cell_mom_j, 0, (size_t)d.mom_cap * sizeof(int), c->stream));
        if (sums) PS_HIP(c, hipMemsetAsync(d.lev_sum, 0, planes * (size_t)d.mom_cap * sizeof(double), c->stream));
        if (P.world > 1) {
            // what every rank's block of the gathered cell sums must say of itself: (first global cell, cells) by rank
            PS_HIP(c, dev_alloc(c, &d.far_plan, far_plan.size()));
            PS_HIP(c, hipMemcpy(d.far_plan, far_plan.data(), far_plan.size() * sizeof(int), hipMemcpyHostToDevice));
        }
    }
    // psamd_update's fixed scratch and result record (behind everything older, which stays where it was)
    PS_HIP(c, dev_alloc(c, &c->upd.hdr, UPDATE_HDR_WORDS));
    PS_HIP(c, dev_alloc(c, &c->upd.tile_live, (size_t)slot_tiles(P.slots_total)));
    PS_HIP(c, dev_alloc(c, &c->upd.own, 1));
    PS_HIP(c, hipMemsetAsync(c->upd.own, 0, sizeof(psamd_update_result), c->stream));
    // psamd_deposit's scratch and result record: a partial per workgroup of tasks at refine 4, the most there are (the
    // compute cells are the plan's: fixed)
    PS_HIP(c, dev_alloc(c, &c->dep.parts, ((size_t)comp_count(P) * 8 + DEPOSIT_WG_TASKS - 1) / DEPOSIT_WG_TASKS));
    PS_HIP(c, dev_alloc(c, &c->dep.own, 1));
    PS_HIP(c, hipMemsetAsync(c->dep.own, 0, sizeof(psamd_deposit_result), c->stream));
    // psamd_sample's counters and result record
    PS_HIP(c, dev_alloc(c, &c->smp.hdr, SAMPLE_HDR_WORDS));
    PS_HIP(c, dev_alloc(c, &c->smp.own, 1));
    PS_HIP(c, hipMemsetAsync(c->smp.own, 0, sizeof(psamd_sample_result), c->stream));
    return PSAMD_OK;
}

// The slab messages' buffers, zeroed, in the table's order (context_params.hpp sized them); beside them what indexes them.
static int alloc_slab_msgs(psamd_ctx *c)
{
    const Geometry &g = c->geo; const DevParams &P = c->P; DeviceState &d = c->d;
    for (int which : MSG_ALLOC_ORDER) {
        SlabMsg &m = c->msg[which];
        if (!m.alloc) continue;
        PS_HIP(c, dev_alloc(c, &m.ptr, m.alloc / sizeof(int)));
        PS_HIP(c, hipMemsetAsync(m.ptr, 0, m.alloc, c->stream));
        const int k = which & 1;
        if (which - k == MSG_HALO_OUT) PS_HIP(c, dev_alloc(c, &c->pack_off[k], (size_t)c->halo_out_cells[k] + 1));
        if (which - k == MSG_HALO_IN) PS_HIP(c, dev_alloc(c, &c->unpack_off[k], (size_t)c->halo_in_cells[k] + 1));
        if (which == MSG_ALLG_IN && (P.flags & PSAMD_FLAG_ALL_PAIRS)) {
            PS_HIP(c, dev_alloc(c, &d.gstart, (size_t)g.num_cells + 1));
            PS_HIP(c, dev_alloc(c, &d.gn, (size_t)g.num_cells + 1));
            PS_HIP(c, hipMemsetAsync(d.gstart, 0, ((size_t)g.num_cells + 1) * sizeof(int), c->stream));
            PS_HIP(c, hipMemsetAsync(d.gn, 0, ((size_t)g.num_cells + 1) * sizeof(int), c->stream));
        }
    }
    const int outbox[5] = {MSG_XFER_OUT, MSG_XFER_OUT + 1, MSG_XFER2_OUT, MSG_XFER2_OUT + 1, MSG_FAR_OUT};
    for (int k = 0; k < 5; k++)
        if (c->msg[outbox[k]].ptr) d.xfer_out[k] = reinterpret_cast<XferRec *>(c->msg[outbox[k]].ptr + MSG_HEADER_WORDS);
    d.allg_in = c->msg[MSG_ALLG_IN].ptr;
    d.status_out = c->msg[MSG_STATUS_OUT].ptr;
    return PSAMD_OK;
}

// From which squared distance on is the fp32 add of EPS2 bit-identical to the
// reference's double add?  Try a few candidates, each checked on the device for
// every float up to the largest squared distance two in-box particles can have.
static int probe_eps_f32(psamd_ctx *c, const psamd_config *cfg)
{
    DevParams &P = c->P;
    if (P.lean_math && cfg->eps2 > 0) {
        const float d2_max = (float)max_d2(c->geo);
        unsigned long long *bad = (unsigned long long *)c->d.fs;   // scratch, zeroed again by init_state
        auto fbits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
        // (below 1.5 x EPS2 the sum lies under 0.5, a binade finer, and the rounding error of (float)EPS2 shows: 838 861 of the floats
        // in [1.25 EPS2, 1.5 EPS2) differ at the reference's EPS2 -- lower multiples are not worth a try)
        for (double mult : {1.5, 2.0, 4.0, 8.0, 16.0, 64.0}) {
            const float from = (float)(mult * cfg->eps2);
            if (!(from < d2_max)) break;
            unsigned long long h_bad = 1;
            PS_HIP(c, hipMemsetAsync(bad, 0, sizeof(unsigned long long), c->stream));
            PS_HIP(c, launch_validate_eps(c->stream, fbits(from), fbits(d2_max), cfg->eps2, P.eps2f, bad));
            PS_HIP(c, hipMemcpyAsync(&h_bad, bad, sizeof h_bad, hipMemcpyDeviceToHost, c->stream));
            PS_HIP(c, hipStreamSynchronize(c->stream));
            if (h_bad == 0) { P.eps_f32_from = from; break; }
        }
    }
    P.slow_below = std::max(P.eps_f32_from, std::nextafterf(P.coll_d2_gate, INFINITY));
    return PSAMD_OK;
}

// The state a fresh context starts from, and the tables that never change.
static int init_state(psamd_ctx *c)
{
    const Geometry &g = c->geo; const DevParams &P = c->P; DeviceState &d = c->d;
    const size_t C = (size_t)P.slots_total, SC = (size_t)P.sorted_cap + 64, LC = (size_t)P.n_local_cells;
    c->wait_policy = P.world > 1 ? 1 : 0;
    if (const char *lim = std::getenv("PSAMD_WAIT_LIMIT_S")) c->wait_limit_s = std::max(0.05, std::atof(lim));
    // init_particles (ps.cpp:722-753): every slot reset, cell = -1
    for (float4 *a : {d.pos4, d.vel4, d.acc4}) PS_HIP(c, hipMemsetAsync(a, 0, std::max<size_t>(C, 1) * sizeof(float4), c->stream));
    PS_HIP(c, hipMemsetAsync(d.pflags, 0, std::max<size_t>(C, 1), c->stream));
    PS_HIP(c, hipMemsetAsync(d.force4, 0, SC * sizeof(float4), c->stream));
    PS_HIP(c, hipMemsetAsync(d.flag_slot, 0, std::max<size_t>(C, 1), c->stream));
    PS_HIP(c, hipMemsetAsync(d.fs, 0, sizeof(FrameScalars), c->stream));
    PS_HIP(c, hipMemsetAsync(d.ctr, 0, sizeof(DevCounters) * COUNTER_COPIES, c->stream));
    PS_HIP(c, hipMemsetAsync(d.cell_count, 0, c->frame_ints * sizeof(int), c->stream));     // (the frame's counts: one allocation)
    PS_HIP(c, hipMemsetAsync(d.cell_start, 0, (LC + 1) * sizeof(int), c->stream));
    PS_HIP(c, launch_fill_int(c->stream, d.cell, -1, C));
    PS_HIP(c, launch_fill_int(c->stream, c->rem.claim, INT32_MAX, C));      // psamd_remove: no slot is claimed between calls
    PS_HIP(c, launch_init_tdata(c->stream, P, d));
    // q_start_fast (ps.cpp:814-871) and the cell table
    g.initial_queues(c->h_qinfo, c->h_queue);
    c->celltab = g.cell_table();
    PS_HIP(c, hipMemcpyAsync(d.celltab, c->celltab.data(), c->celltab.size() * sizeof(CellInfo), hipMemcpyHostToDevice, c->stream));
    {   // k_sort_cells' order of the own cells: the cells of one segment (they share its slots, so their gathers share
        // cache lines) side by side -- one XCD's L2 then sees a segment's lines once
        const int cell_off = P.reg_first[0] * g.G * g.G;
        std::vector<int> order((size_t)std::max(P.n_own_cells, 1), 0);
        for (int lc = 0; lc < P.n_own_cells; lc++) order[(size_t)lc] = lc;
        std::stable_sort(order.begin(), order.begin() + P.n_own_cells, [&](int a, int b) {
            const CellInfo &x = c->celltab[(size_t)(a + cell_off)], &y = c->celltab[(size_t)(b + cell_off)];
            if (x.chunk != y.chunk) return x.chunk < y.chunk;
            if (x.seg_type != y.seg_type) return x.seg_type < y.seg_type;
            return x.seg_tid < y.seg_tid;
        });
        PS_HIP(c, dev_alloc(c, &d.cell_order, order.size()));
        PS_HIP(c, hipMemcpy(d.cell_order, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    return push_queues(c);       // (host_queues_valid: the mirror is what the device now holds)
}

int psamd_create(const psamd_config *cfg, psamd_ctx **out)
{
    if (!cfg || !out) return PSAMD_ERR_INVALID_ARG;
    *out = nullptr;
    psamd_ctx *c = new (std::nothrow) psamd_ctx();
    if (!c) return PSAMD_ERR_OUT_OF_MEMORY;
    *out = c;  // returned even on failure so psamd_last_error can explain; caller destroys it
    if (!c->geo.init(*cfg)) return fail(c, PSAMD_ERR_INVALID_ARG, "bad configuration (chunk_dim >= 3, sizes > 0, container < 2^31)");
    // (derive_context_params' first two refusals, also ahead of the device's: a bad rank or plan is told apart from a missing GPU)
    std::string why;
    if (const int rc = rank_plan(*cfg, c->geo, c->plan, why)) return fail(c, rc, why);

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(c, PSAMD_ERR_NO_DEVICE, "hipGetDeviceCount found none");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(c, PSAMD_ERR_NO_DEVICE, "device ordinal out of range");
    PS_HIP(c, hipSetDevice(cfg->device));
    PS_HIP(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    PS_HIP(c, hipStreamCreateWithFlags(&c->d.side_stream, hipStreamNonBlocking));
    PS_HIP(c, hipEventCreateWithFlags(&c->d.ev_fork, hipEventDisableTiming));
    PS_HIP(c, hipEventCreateWithFlags(&c->d.ev_join, hipEventDisableTiming));

    ContextParams cp;
    int rc = derive_context_params(*cfg, c->geo, std::getenv("PSAMD_ONE_PASS") != nullptr, cp, why);
    if (rc != PSAMD_OK) return fail(c, rc, why);
    c->P = cp.P; c->S = cp.S; c->have_interior = cp.have_interior;
    c->frame_ints = cp.frame_ints; c->d.ops_cap = cp.ops_cap; c->d.moves_cap = cp.moves_cap; c->d.lev = cp.lev;
    for (int k = 0; k < 2; k++) { c->halo_out_c0[k] = cp.halo_out_c0[k]; c->halo_out_cells[k] = cp.halo_out_cells[k]; c->halo_in_cells[k] = cp.halo_in_cells[k]; }
    for (int w = 0; w < MSG_COUNT; w++) { c->msg[w].bytes = cp.msg[w].bytes; c->msg[w].alloc = cp.msg[w].alloc; }
    rc = alloc_step_arrays(c, cp.far_plan);
    if (rc == PSAMD_OK) rc = alloc_slab_msgs(c);
    if (rc == PSAMD_OK) rc = probe_eps_f32(c, cfg);      // (on the device: after the allocations, as ever)
    if (rc != PSAMD_OK) return rc;
    // the pair stage cut in two: the probed parameters, each pass's own ranges
    c->P_int = c->P_rest = c->P;
    for (int k = 0; k < 3; k++) {
        c->P_int.comp_lo[k] = cp.int_lo[k]; c->P_int.comp_hi[k] = cp.int_hi[k];
        c->P_rest.comp_lo[k] = cp.rest_lo[k]; c->P_rest.comp_hi[k] = cp.rest_hi[k];
    }
    return init_state(c);
}

int psamd_destroy(psamd_ctx *c)
{
    if (!c) return PSAMD_OK;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    drop_graphs(c);
    for (void *p : c->allocs) (void)hipFree(p);
    if (c->staging) (void)hipFree(c->staging);
    for (const EntryScratch &e : {c->inj.e, c->rem.e})
        for (void *p : {(void *)e.ent, (void *)e.tcount, (void *)e.tile_out}) if (p) (void)hipFree(p);
    for (void *p : {(void *)c->prb.code, (void *)c->prb.order, (void *)c->upd.code, c->nbr.block, c->grp.block, c->knn.block}) if (p) (void)hipFree(p);
    if (c->h_fs) (void)hipHostFree(c->h_fs);
    if (c->ev_made) for (auto &set : c->ev) for (auto &e : set) (void)hipEventDestroy(e);
    if (c->d.ev_fork) (void)hipEventDestroy(c->d.ev_fork);
    if (c->d.ev_join) (void)hipEventDestroy(c->d.ev_join);
    if (c->d.side_stream) (void)hipStreamDestroy(c->d.side_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return PSAMD_OK;
}

static void fill_sizes(const Geometry &g, psamd_sizes *o)
{
    std::memset(o, 0, sizeof *o);
    o->grid_dim = g.G; o->num_cells = g.num_cells; o->num_chunks = g.num_chunks;
    o->cells_per_chunk = g.cells_per_chunk; o->max_per_cell = g.max_per_cell; o->max_per_chunk = g.max_per_chunk;
    o->container_size = g.container; o->queue_info_size = g.queue_infos;
    o->n_chunkgrid = (int64_t)g.num_chunks * (1 + (int64_t)g.max_per_chunk);
    o->n_cellgrid = (int64_t)g.num_cells * (1 + (int64_t)g.max_per_cell);
    o->n_pkgdistrib = g.num_chunks * 27;
    for (int k = 0; k < 4; k++) { o->seg_count[k] = g.seg_count[k]; o->seg_size_t[k] = g.seg_size_t[k]; o->seg_size[k] = g.seg_size[k]; }
}

int psamd_describe(const psamd_config *cfg, psamd_sizes *sizes, int32_t *cell_table3, int32_t *pkg,
                   void *queue_info24, int32_t *queue)
{
    if (!cfg) return PSAMD_ERR_INVALID_ARG;
    Geometry g;
    if (!g.init(*cfg)) return PSAMD_ERR_INVALID_ARG;
    if (sizes) fill_sizes(g, sizes);
    if (cell_table3)
        for (int i = 0; i < g.num_cells; i++) {
            const CellInfo ci = g.cell_info(i);
            cell_table3[3 * i] = ci.chunk; cell_table3[3 * i + 1] = ci.seg_type; cell_table3[3 * i + 2] = ci.seg_tid;
        }
    if (pkg) for (int ch = 0; ch < g.num_chunks; ch++) g.chunk_segments(ch, (Pair *)pkg + (size_t)ch * 27);
    if (queue_info24 || queue) {
        std::vector<QueueInfo> qi;
        std::vector<int32_t> q;
        g.initial_queues(qi, q);
        if (queue_info24) std::memcpy(queue_info24, qi.data(), qi.size() * sizeof(QueueInfo));
        if (queue) std::memcpy(queue, q.data(), q.size() * sizeof(int32_t));
    }
    return PSAMD_OK;
}

int psamd_get_sizes(const psamd_ctx *c, psamd_sizes *o)
{
    if (!c || !o) return PSAMD_ERR_INVALID_ARG;
    fill_sizes(c->geo, o);
    return PSAMD_OK;
}

int psamd_get_config(const psamd_ctx *c, psamd_config *o)
{
    if (!c || !o) return PSAMD_ERR_INVALID_ARG;
    *o = c->geo.cfg;
    return PSAMD_OK;
}

int psamd_slab_plan_describe(const psamd_config *cfg, psamd_slab_plan *o)
{
    if (!cfg || !o) return PSAMD_ERR_INVALID_ARG;
    Geometry g;
    if (!g.init(*cfg)) return PSAMD_ERR_INVALID_ARG;
    SlabPlan p;
    std::string why;
    if (const int rc = rank_plan(*cfg, g, p, why)) return rc;
    std::memset(o, 0, sizeof *o);
    o->world = p.world; o->rank = p.rank; o->grid_dim = p.G;
    o->cut_lo = p.cut_lo; o->cut_hi = p.cut_hi; o->state_lo = p.state_lo; o->state_hi = p.state_hi;
    o->below_lo = p.below_lo; o->below_hi = p.below_hi; o->above_lo = p.above_lo; o->above_hi = p.above_hi;
    o->lentin_lo = p.lentin_lo; o->lentin_hi = p.lentin_hi; o->lentout_lo = p.lentout_lo; o->lentout_hi = p.lentout_hi;
    o->send_up_lo = p.send_up_lo; o->send_up_hi = p.send_up_hi; o->send_down_lo = p.send_down_lo; o->send_down_hi = p.send_down_hi;
    for (int t = 0; t < 4; t++) { o->slot_lo[t] = p.slot_lo[t]; o->slot_hi[t] = p.slot_hi[t]; o->rec_lo[t] = p.rec_lo[t]; o->rec_hi[t] = p.rec_hi[t]; }
    o->up_rank = p.up_rank; o->down_rank = p.down_rank;
    return PSAMD_OK;
}

int psamd_get_slab_plan(const psamd_ctx *c, psamd_slab_plan *o)
{
    if (!c || !o) return PSAMD_ERR_INVALID_ARG;
    return psamd_slab_plan_describe(&c->geo.cfg, o);
}

}  // extern "C"
