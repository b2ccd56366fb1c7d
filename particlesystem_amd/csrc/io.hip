// io.hip -- state in and out of a context: fill / upload / download, export, inject, snapshot, the slab message
// buffers, and the debug / self-test calls.  Nothing here enqueues a stage of the step.
#include <random>

#include "context.hpp"

static int ensure_staging(psamd_ctx *c, size_t bytes)
{
    if (bytes <= c->staging_bytes) return PSAMD_OK;
    if (c->staging) (void)hipFree(c->staging);
    c->staging = nullptr; c->staging_bytes = 0;
    PS_HIP(c, hipMalloc(&c->staging, bytes));
    c->staging_bytes = bytes;
    return PSAMD_OK;
}

// The device keeps the queue array for the owned segments only, back to back (like the slot
// arrays); the host mirrors are whole-container arrays whose foreign parts are never used.
template <typename F>
static void for_owned_ranges(const psamd_ctx *c, F fn)
{
    size_t off = 0;
    for (int t = 0; t < 4; t++) {
        const int n = c->P.slot_n[t];
        if (n > 0) fn((size_t)c->P.slot_lo[t], (size_t)n, off);
        off += (size_t)n;
    }
}

namespace psamd {
int pull_queues(psamd_ctx *c)   // device -> host mirror
{
    if (c->host_queues_valid) return PSAMD_OK;
    PS_HIP(c, hipStreamSynchronize(c->stream));
    PS_HIP(c, hipMemcpy(c->h_qinfo.data(), c->d.qinfo, c->h_qinfo.size() * sizeof(QueueInfo), hipMemcpyDeviceToHost));
    hipError_t e = hipSuccess;
    for_owned_ranges(c, [&](size_t lo, size_t n, size_t off) {
        if (e == hipSuccess) e = hipMemcpy(c->h_queue.data() + lo, c->d.queue + off, n * sizeof(int32_t), hipMemcpyDeviceToHost);
    });
    PS_HIP(c, e);
    c->host_queues_valid = true;
    return PSAMD_OK;
}

int push_queues(psamd_ctx *c)   // host mirror -> device
{
    PS_HIP(c, hipMemcpyAsync(c->d.qinfo, c->h_qinfo.data(), c->h_qinfo.size() * sizeof(QueueInfo), hipMemcpyHostToDevice, c->stream));
    hipError_t e = hipSuccess;
    for_owned_ranges(c, [&](size_t lo, size_t n, size_t off) {
        if (e == hipSuccess) e = hipMemcpyAsync(c->d.queue + off, c->h_queue.data() + lo, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
    });
    PS_HIP(c, e);
    PS_HIP(c, hipStreamSynchronize(c->stream));
    return PSAMD_OK;
}
}  // namespace psamd

// q_remove on the host mirror (app_common.cu:305-339), used by the fill stage only
static int host_q_remove(psamd_ctx *c, int seg_type, int seg_tid)
{
    QueueInfo &q = c->h_qinfo[(size_t)c->geo.segment_record(seg_type, seg_tid)];
    if (q.count <= 0) return -1;
    const int pos = q.front;
    if (q.count == 1) { q.front = -1; q.rear = -1; }
    else if (q.front == q.rloc + q.seg_size - 1) q.front = q.rloc;
    else q.front++;
    q.count--;
    const int item = c->h_queue[(size_t)pos];
    c->h_queue[(size_t)pos] = -1;
    return item;
}

extern "C" {

int psamd_uniform_cloud(const psamd_ctx *c, int64_t n, uint32_t seed, float *xyz)
{
    if (!c || !xyz || n < 0) return PSAMD_ERR_INVALID_ARG;
    // ps.cpp:974-1028 draws r*sign*range per axis from a random_device-seeded mt19937;
    // a fixed seed and one uniform draw per axis give the same distribution reproducibly
    const float half = (float)((c->geo.G / 2) * c->geo.cfg.cell_size);
    std::mt19937 gen(seed);
    std::uniform_real_distribution<float> dist(-half, half);
    for (int64_t i = 0; i < n; i++) {
        // a draw can land exactly on a face that belongs to the neighbouring (missing)
        // cell: -half on the negated axes y and z, +half (float rounding) on x; draw again
        int cell;
        do {
            xyz[3 * i] = dist(gen); xyz[3 * i + 1] = dist(gen); xyz[3 * i + 2] = dist(gen);
        } while (!c->geo.locate(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], cell));
    }
    return PSAMD_OK;
}

int psamd_fill_particles(psamd_ctx *c, int64_t n, const float *xyz, const float *vxyz, const float *w,
                         const float *age, const float *fert_age, int32_t *ids_out, int64_t *n_done)
{
    if (n_done) *n_done = 0;
    if (!c || n < 0 || (n > 0 && !xyz)) return PSAMD_ERR_INVALID_ARG;
    if (n == 0) return PSAMD_OK;
    int rc = pull_queues(c);
    if (rc != PSAMD_OK) return rc;
    const Geometry &g = c->geo;
    struct Rec { float4 p, v, a; int cell; };
    std::vector<int32_t> ids((size_t)n);
    std::vector<Rec> recs((size_t)n);
    int64_t done = 0, placed = 0;
    int status = PSAMD_OK;
    for (; done < n; done++) {
        const float x = xyz[3 * done], y = xyz[3 * done + 1], z = xyz[3 * done + 2];
        int cell;
        if (!g.locate(x, y, z, cell)) { status = fail(c, PSAMD_ERR_OUTSIDE_BOX, "fill_particles"); break; }
        const CellInfo &ci = c->celltab[(size_t)cell];
        Rec &r = recs[(size_t)done];
        // a slab places only the particles of its own segments (their queues are its own: the
        // order among them is the reference's), the others are their owners' business
        if (!owns_record(c->P, g.segment_record(ci.seg_type, ci.seg_tid))) { ids[(size_t)done] = -1; r.cell = -1; continue; }
        const int nid = host_q_remove(c, ci.seg_type, ci.seg_tid);
        if (nid < 0) { status = fail(c, PSAMD_ERR_QUEUE_EMPTY, "fill_particles"); break; }
        ids[(size_t)done] = nid;
        placed++;
        r.cell = cell;
        r.p = make_float4(x, y, z, w ? w[done] : (float)g.cfg.particle_weight);
        r.v = make_float4(vxyz ? vxyz[3 * done] : 0.f, vxyz ? vxyz[3 * done + 1] : 0.f, vxyz ? vxyz[3 * done + 2] : 0.f,
                          age ? age[done] : 0.f);
        r.a = make_float4(0.f, 0.f, 0.f, fert_age ? fert_age[done] : 0.f);
    }
    // create_particle_s overwrites every field of the slot (app.cu:189-208): ship the
    // records once and let a kernel drop them into their slots
    if (done > 0) {
        const size_t m = (size_t)done;
        std::vector<float4> hp(m), hv(m), ha(m);
        std::vector<int> hc(m);
        for (size_t k = 0; k < m; k++) { hp[k] = recs[k].p; hv[k] = recs[k].v; ha[k] = recs[k].a; hc[k] = recs[k].cell; }
        const size_t bytes = m * (3 * sizeof(float4) + 2 * sizeof(int));
        rc = ensure_staging(c, bytes);
        if (rc != PSAMD_OK) return rc;
        char *base = (char *)c->staging;
        float4 *dp = (float4 *)base, *dv = dp + m, *da = dv + m;
        int *dc = (int *)(da + m), *di = dc + m;
        PS_HIP(c, hipMemcpyAsync(dp, hp.data(), m * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        PS_HIP(c, hipMemcpyAsync(dv, hv.data(), m * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        PS_HIP(c, hipMemcpyAsync(da, ha.data(), m * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        PS_HIP(c, hipMemcpyAsync(dc, hc.data(), m * sizeof(int), hipMemcpyHostToDevice, c->stream));
        PS_HIP(c, hipMemcpyAsync(di, ids.data(), m * sizeof(int), hipMemcpyHostToDevice, c->stream));
        PS_HIP(c, launch_place(c->stream, c->P, (int)done, di, dp, dv, da, dc, c->d));
        PS_HIP(c, hipStreamSynchronize(c->stream));
    }
    rc = push_queues(c);
    if (rc != PSAMD_OK) return rc;
    if (ids_out) std::copy(ids.begin(), ids.begin() + done, ids_out);
    if (n_done) *n_done = done;
    if (c->live_bound >= 0) c->live_bound += placed;
    c->grid_built = false; c->pairs_done = false; c->slab_stage = 0;
    return status;
}

int psamd_upload_particles(psamd_ctx *c, const void *p72, int64_t first, int64_t count)
{
    if (!c || !p72 || first < 0 || count < 0 || first + count > c->geo.container) return PSAMD_ERR_INVALID_ARG;
    if (count == 0) return PSAMD_OK;
    int rc = ensure_staging(c, (size_t)count * 72);
    if (rc != PSAMD_OK) return rc;
    PS_HIP(c, hipMemcpyAsync(c->staging, p72, (size_t)count * 72, hipMemcpyHostToDevice, c->stream));
    // odd grids are not centred (G/2 is an integer division): allow the longer half
    const float half_box = (float)((c->geo.G - c->geo.G / 2) * c->geo.cfg.cell_size);
    PS_HIP(c, launch_unpack_aos(c->stream, c->P, c->staging, (int)first, (int)count, half_box, c->d));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    c->grid_built = false; c->pairs_done = false; c->slab_stage = 0;
    c->live_bound = -1;
    return check_device_errors(c);
}

int psamd_download_particles(psamd_ctx *c, void *p72, int64_t first, int64_t count)
{
    if (!c || !p72 || first < 0 || count < 0 || first + count > c->geo.container) return PSAMD_ERR_INVALID_ARG;
    if (count == 0) return PSAMD_OK;
    int rc = ensure_staging(c, (size_t)count * 72);
    if (rc != PSAMD_OK) return rc;
    PS_HIP(c, launch_pack_aos(c->stream, c->P, c->staging, (int)first, (int)count, c->d));
    PS_HIP(c, hipMemcpyAsync(p72, c->staging, (size_t)count * 72, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    return PSAMD_OK;
}

int psamd_download_tdata(psamd_ctx *c, void *t24, int64_t first, int64_t count)
{
    if (!c || !t24 || first < 0 || count < 0 || first + count > c->geo.container) return PSAMD_ERR_INVALID_ARG;
    if (count == 0) return PSAMD_OK;
    if (!c->tdata_mirror) return fail(c, PSAMD_ERR_STATE, "the T_DATA mirror is off (psamd_set_tdata_mirror): build_grid has not been writing the rows");
    PS_HIP(c, hipStreamSynchronize(c->stream));
    // rows of slots another rank owns: as init_particles left them (id, zeros; ps.cpp:743-748)
    uint32_t *out = (uint32_t *)t24;
    if (c->P.world > 1)
        for (int64_t i = 0; i < count; i++) { uint32_t *r = out + 6 * i; r[0] = (uint32_t)(first + i); r[1] = r[2] = r[3] = r[4] = r[5] = 0u; }
    hipError_t e = hipSuccess;
    for_owned_ranges(c, [&](size_t lo, size_t n, size_t off) {
        const int64_t a = std::max<int64_t>(first, (int64_t)lo), b = std::min<int64_t>(first + count, (int64_t)(lo + n));
        if (a < b && e == hipSuccess)
            e = hipMemcpy(out + 6 * (a - first), c->d.tdata + 6 * (off + (size_t)(a - (int64_t)lo)), (size_t)(b - a) * 24, hipMemcpyDeviceToHost);
    });
    PS_HIP(c, e);
    return PSAMD_OK;
}

int psamd_upload_queues(psamd_ctx *c, const void *qi, const int32_t *queue)
{
    if (!c || !qi || !queue) return PSAMD_ERR_INVALID_ARG;
    std::memcpy(c->h_qinfo.data(), qi, c->h_qinfo.size() * sizeof(QueueInfo));
    std::memcpy(c->h_queue.data(), queue, c->h_queue.size() * sizeof(int32_t));
    c->host_queues_valid = true;
    return push_queues(c);
}

int psamd_download_queues(psamd_ctx *c, void *qi, int32_t *queue)
{
    if (!c || !qi || !queue) return PSAMD_ERR_INVALID_ARG;
    int rc = pull_queues(c);
    if (rc != PSAMD_OK) return rc;
    std::memcpy(qi, c->h_qinfo.data(), c->h_qinfo.size() * sizeof(QueueInfo));
    std::memcpy(queue, c->h_queue.data(), c->h_queue.size() * sizeof(int32_t));
    return PSAMD_OK;
}

// Rebuild the reference's fixed-stride lists from the compact sorted arrays.  start[] is
// indexed by the own LOCAL cells (region 0); local cell lc is global cell lc + cell_off.
static int fetch_sorted(psamd_ctx *c, std::vector<int> &start, std::vector<int> &ids)
{
    if (!c->grid_built) return fail(c, PSAMD_ERR_STATE, "grid lists requested before build_grid");
    start.resize((size_t)c->P.n_own_cells + 1);
    PS_HIP(c, hipStreamSynchronize(c->stream));
    PS_HIP(c, hipMemcpy(start.data(), c->d.cell_start, start.size() * sizeof(int), hipMemcpyDeviceToHost));
    ids.resize((size_t)std::max(start.back(), 1));
    PS_HIP(c, hipMemcpy(ids.data(), c->d.sorted_id, (size_t)start.back() * sizeof(int), hipMemcpyDeviceToHost));
    return PSAMD_OK;
}

int psamd_download_cellgrid(psamd_ctx *c, int32_t *out)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    std::vector<int> start, ids;
    int rc = fetch_sorted(c, start, ids);
    if (rc != PSAMD_OK) return rc;
    const Geometry &g = c->geo;
    const size_t stride = 1 + (size_t)g.max_per_cell;
    const int cell_off = c->P.reg_first[0] * g.G * g.G;
    std::memset(out, 0, sizeof(int32_t) * stride * (size_t)g.num_cells);
    for (int lc = 0; lc < c->P.n_own_cells; lc++) {
        const int n = std::min(start[(size_t)lc + 1] - start[(size_t)lc], g.max_per_cell);
        int32_t *row = out + stride * (size_t)(lc + cell_off);
        row[0] = n;
        for (int k = 0; k < n; k++) row[1 + k] = ids[(size_t)start[(size_t)lc] + k];
    }
    return PSAMD_OK;
}

int psamd_download_force_counts(psamd_ctx *c, int32_t *out)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    if (!c->pairs_done) return fail(c, PSAMD_ERR_STATE, "force counts requested before the pair pass of this frame");
    PS_HIP(c, hipStreamSynchronize(c->stream));
    const Geometry &g = c->geo;
    const DevParams &P = c->P;
    const bool two = P.two_pass && P.lean_math;
    std::memset(out, 0, sizeof(int32_t) * (size_t)g.num_cells);
    std::vector<int> v((size_t)P.n_local_cells + 1);
    if (two) PS_HIP(c, hipMemcpy(v.data(), c->d.active_count, sizeof(int) * (size_t)P.n_local_cells, hipMemcpyDeviceToHost));
    else PS_HIP(c, hipMemcpy(v.data(), c->d.cell_start, sizeof(int) * ((size_t)P.n_local_cells + 1), hipMemcpyDeviceToHost));
    for (int j = 0; j < comp_count(P); j++) {
        const int lc = comp_cell(P, j);
        // one-pass modes evaluate every particle's sum (and discard what is not used)
        out[global_of_local(P, lc)] = two ? v[(size_t)lc] : std::min(v[(size_t)lc + 1] - v[(size_t)lc], g.max_per_cell);
    }
    return PSAMD_OK;
}

int psamd_download_chunkgrid(psamd_ctx *c, int32_t *out)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    std::vector<int> start, ids;
    int rc = fetch_sorted(c, start, ids);
    if (rc != PSAMD_OK) return rc;
    const Geometry &g = c->geo;
    const size_t stride = 1 + (size_t)g.max_per_chunk;
    const int cell_off = c->P.reg_first[0] * g.G * g.G;
    std::memset(out, 0, sizeof(int32_t) * stride * (size_t)g.num_chunks);
    // the reference appends in slot order (ps.cpp:1502-1508): per chunk, ids ascending,
    // including the ones the cell-overflow rule then killed (stored as ~id in fetch order)
    std::vector<std::vector<int>> per((size_t)g.num_chunks);
    for (int lc = 0; lc < c->P.n_own_cells; lc++) {
        auto &v = per[(size_t)c->celltab[(size_t)(lc + cell_off)].chunk];
        for (int k = start[(size_t)lc]; k < start[(size_t)lc + 1]; k++) v.push_back(ids[(size_t)k]);
    }
    for (int ch = 0; ch < g.num_chunks; ch++) {
        auto &v = per[(size_t)ch];
        std::sort(v.begin(), v.end());
        int32_t *row = out + stride * (size_t)ch;
        row[0] = (int32_t)v.size();
        const size_t n = std::min(v.size(), (size_t)g.max_per_chunk);
        for (size_t k = 0; k < n; k++) row[1 + k] = v[k];
    }
    return PSAMD_OK;
}

int psamd_get_pkgdistrib(const psamd_ctx *c, int32_t *out)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    for (int ch = 0; ch < c->geo.num_chunks; ch++) c->geo.chunk_segments(ch, (Pair *)out + (size_t)ch * 27);
    return PSAMD_OK;
}

int psamd_get_cell_table(const psamd_ctx *c, int32_t *out)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    for (int i = 0; i < c->geo.num_cells; i++) {
        out[3 * i] = c->celltab[(size_t)i].chunk;
        out[3 * i + 1] = c->celltab[(size_t)i].seg_type;
        out[3 * i + 2] = c->celltab[(size_t)i].seg_tid;
    }
    return PSAMD_OK;
}

int psamd_get_gridmax(psamd_ctx *c, int32_t out2[2])
{
    if (!c || !out2) return PSAMD_ERR_INVALID_ARG;
    // inside a frame (after build_grid) the device's record is the frame's; once calc_forces has run the device's record
    // belongs to the next frame already and the step's scalars are in the host's copy (ps.cpp:1900 reads hostGridMax
    // between the stages; the reference's array keeps the build's values until the next init_iframe)
    const int rc = drain_scalars(c);
    if (rc != PSAMD_OK && !c->grid_built) return rc;
    if (c->grid_built) {
        FrameScalars fs{};
        PS_HIP(c, hipMemcpy(&fs, c->d.fs, sizeof fs, hipMemcpyDeviceToHost));
        out2[0] = fs.gridmax[0]; out2[1] = fs.gridmax[1];
        c->live_at_build = fs.live;
    } else { out2[0] = c->last.gridmax[0]; out2[1] = c->last.gridmax[1]; }
    return PSAMD_OK;
}

int psamd_slab_buffers_get(psamd_ctx *c, psamd_slab_buffers *o)
{
    if (!c || !o) return PSAMD_ERR_INVALID_ARG;
    std::memset(o, 0, sizeof *o);
    const SlabMsg *m = c->msg;
    for (int k = 0; k < 2; k++) {
        o->halo_out[k] = m[MSG_HALO_OUT + k].ptr; o->halo_out_bytes[k] = (int64_t)m[MSG_HALO_OUT + k].bytes;
        o->halo_in[k] = m[MSG_HALO_IN + k].ptr; o->halo_in_bytes[k] = (int64_t)m[MSG_HALO_IN + k].bytes;
        o->xfer_out[k] = m[MSG_XFER_OUT + k].ptr; o->xfer_in[k] = m[MSG_XFER_IN + k].ptr;
        o->xfer2_out[k] = m[MSG_XFER2_OUT + k].ptr; o->xfer2_in[k] = m[MSG_XFER2_IN + k].ptr;
    }
    o->force_out = m[MSG_FORCE_OUT].ptr; o->force_out_bytes = (int64_t)m[MSG_FORCE_OUT].bytes;
    o->force_in = m[MSG_FORCE_IN].ptr; o->force_in_bytes = (int64_t)m[MSG_FORCE_IN].bytes;
    o->xfer_bytes = (int64_t)m[MSG_XFER_OUT].bytes; o->xfer2_bytes = (int64_t)m[MSG_XFER2_OUT].bytes;
    o->xfer_bytes_max = c->P.world > 1 ? (int64_t)xfer_msg_bytes((size_t)c->P.xfer_cap_max + 1) : 0;
    // (the *_bytes of the all-gathered messages are one rank's part)
    o->status_out = m[MSG_STATUS_OUT].ptr; o->status_in = m[MSG_STATUS_IN].ptr; o->status_bytes = (int64_t)m[MSG_STATUS_OUT].bytes;
    o->allg_out = m[MSG_ALLG_OUT].ptr; o->allg_in = m[MSG_ALLG_IN].ptr; o->allg_bytes = (int64_t)m[MSG_ALLG_OUT].bytes;
    o->far_out = m[MSG_FAR_OUT].ptr; o->far_in = m[MSG_FAR_IN].ptr; o->far_bytes = (int64_t)m[MSG_FAR_OUT].bytes;
    return PSAMD_OK;
}

// message `which` of the ABI to or from the host: at most the bytes that travel now
static int msg_copy(psamd_ctx *c, int which, void *host, int64_t bytes, hipMemcpyKind kind)
{
    if (!c || !host || which < 0 || which >= MSG_COUNT || bytes < 0 || (size_t)bytes > c->msg[which].bytes) return PSAMD_ERR_INVALID_ARG;
    if (bytes == 0) return PSAMD_OK;
    const bool up = kind == hipMemcpyHostToDevice;
    PS_HIP(c, hipMemcpyAsync(up ? c->msg[which].ptr : host, up ? host : c->msg[which].ptr, (size_t)bytes, kind, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    return PSAMD_OK;
}

int psamd_slab_msg_download(psamd_ctx *c, int which, void *host, int64_t bytes) { return msg_copy(c, which, host, bytes, hipMemcpyDeviceToHost); }
int psamd_slab_msg_upload(psamd_ctx *c, int which, const void *host, int64_t bytes) { return msg_copy(c, which, (void *)host, bytes, hipMemcpyHostToDevice); }

int psamd_get_counters(psamd_ctx *c, psamd_counters *o)
{
    if (!c || !o) return PSAMD_ERR_INVALID_ARG;
    (void)drain_scalars(c, true);                // (steps / particles_processed count every step enqueued; a step's verdict is psamd_synchronize's to report)
    DevCounters copies[COUNTER_COPIES];
    PS_HIP(c, hipMemcpy(copies, c->d.ctr, sizeof copies, hipMemcpyDeviceToHost));
    DevCounters d{};
    for (const DevCounters &k : copies) {
        d.deaths_age += k.deaths_age; d.deaths_collision += k.deaths_collision; d.survives += k.survives;
        d.integrated += k.integrated; d.relocations += k.relocations; d.relocations_lost += k.relocations_lost;
        d.births += k.births; d.births_failed += k.births_failed; d.cell_overflow_kills += k.cell_overflow_kills;
    }
    o->deaths_age = (int64_t)d.deaths_age; o->deaths_collision = (int64_t)d.deaths_collision;
    o->survives = (int64_t)d.survives; o->integrated = (int64_t)d.integrated;
    o->relocations = (int64_t)d.relocations; o->relocations_lost = (int64_t)d.relocations_lost;
    o->births = (int64_t)d.births; o->births_failed = (int64_t)d.births_failed;
    o->cell_overflow_kills = (int64_t)d.cell_overflow_kills;
    o->steps = c->steps_total;
    o->particles_processed = c->processed_total;
    o->max_ops_one_queue = c->max_bucket_seen;
    return PSAMD_OK;
}

int psamd_live_count(psamd_ctx *c, int64_t *out)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    PS_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<int> cells((size_t)std::max(c->P.slots_total, 1));
    PS_HIP(c, hipMemcpy(cells.data(), c->d.cell, (size_t)c->P.slots_total * sizeof(int), hipMemcpyDeviceToHost));
    int64_t n = 0;
    for (int i = 0; i < c->P.slots_total; i++) n += (cells[(size_t)i] >= 0 && cells[(size_t)i] < c->geo.num_cells) ? 1 : 0;
    *out = n;
    return PSAMD_OK;
}

int psamd_device_view_get(psamd_ctx *c, psamd_device_view *o)
{
    if (!c || !o) return PSAMD_ERR_INVALID_ARG;
    o->pos4 = c->d.pos4; o->vel4 = c->d.vel4; o->acc4 = c->d.acc4; o->cell = c->d.cell; o->pflags = c->d.pflags;
    o->sorted_id = c->d.sorted_id; o->snap_soa = c->d.snap_soa; o->sorted_cap = c->P.sorted_cap; o->force4 = c->d.force4; o->cell_start = c->d.cell_start;
    o->container_size = c->P.slots_total; o->num_cells = c->P.n_own_cells;
    o->live = c->live_at_build;
    o->stream = (void *)c->stream;
    return PSAMD_OK;
}

// ---- getting frames out (export.hip) ----
static const uint32_t export_bits[5] = {PSAMD_EXPORT_POS, PSAMD_EXPORT_VEL, PSAMD_EXPORT_ACC, PSAMD_EXPORT_ID, PSAMD_EXPORT_CELL};
static const size_t export_size[5] = {sizeof(float4), sizeof(float4), sizeof(float4), sizeof(int32_t), sizeof(int32_t)};

// device: the kernel stores to the arrays (float4 and int32 stores want their natural alignment); host arrays are copied into
static int export_args(psamd_ctx *c, uint32_t fields, void *const ptr[5], int64_t capacity, bool device)
{
    if (fields & ~PSAMD_EXPORT_ALL) return fail(c, PSAMD_ERR_INVALID_ARG, "export: unknown field bits");
    if (capacity < 0) return fail(c, PSAMD_ERR_INVALID_ARG, "export: capacity < 0");
    for (int k = 0; k < 5; k++)
        if ((fields & export_bits[k]) && (!ptr[k] || (device && (uintptr_t)ptr[k] % export_size[k] != 0)))
            return fail(c, PSAMD_ERR_INVALID_ARG, "export: a field asked for has a null or misaligned pointer");
    return PSAMD_OK;
}

static ExportFields export_fields(uint32_t fields, void *const ptr[5])
{
    void *p[5];
    for (int k = 0; k < 5; k++) p[k] = (fields & export_bits[k]) ? ptr[k] : nullptr;
    return ExportFields{(float4 *)p[0], (float4 *)p[1], (float4 *)p[2], (int *)p[3], (int *)p[4]};
}

int psamd_export_live(psamd_ctx *c, const psamd_export *spec)
{
    if (!c || !spec) return PSAMD_ERR_INVALID_ARG;
    if (c->wedged) return refuse_wedged(c);
    void *const ptr[5] = {spec->pos4, spec->vel4, spec->acc4, spec->id, spec->cell};
    if (spec->reserved != 0) return fail(c, PSAMD_ERR_INVALID_ARG, "export: reserved must be 0");
    const int rc = export_args(c, spec->fields, ptr, spec->capacity, true);
    if (rc != PSAMD_OK) return rc;
    PS_HIP(c, launch_export_live(c->stream, c->P, c->d, export_fields(spec->fields, ptr), spec->capacity,
                                 spec->count_dev ? spec->count_dev : &c->d.exp_out->count,
                                 spec->stats_dev ? spec->stats_dev : &c->d.exp_out->stats));
    return PSAMD_OK;
}

int psamd_download_live(psamd_ctx *c, uint32_t fields, void *pos4, void *vel4, void *acc4, int32_t *id, int32_t *cell,
                        int64_t capacity, int64_t *count)
{
    if (!c || !count) return PSAMD_ERR_INVALID_ARG;
    if (c->wedged) return refuse_wedged(c);
    void *const host[5] = {pos4, vel4, acc4, id, cell};
    int rc = export_args(c, fields, host, capacity, false);
    if (rc != PSAMD_OK) return rc;
    // the chosen fields of at most min(capacity, owned slots) particles, one after the other in the staging buffer
    const int64_t n = std::min<int64_t>(capacity, c->P.slots_total);
    size_t off[5] = {0, 0, 0, 0, 0}, bytes = 0;
    for (int k = 0; k < 5; k++)
        if (fields & export_bits[k]) { off[k] = bytes; bytes += ((size_t)n * export_size[k] + 255) / 256 * 256; }
    rc = ensure_staging(c, std::max<size_t>(bytes, 256));
    if (rc != PSAMD_OK) return rc;
    void *dev[5];
    for (int k = 0; k < 5; k++) dev[k] = (char *)c->staging + off[k];
    PS_HIP(c, launch_export_live(c->stream, c->P, c->d, export_fields(fields, dev), n, &c->d.exp_out->count, &c->d.exp_out->stats));
    int64_t total = 0;
    PS_HIP(c, hipMemcpyAsync(&total, &c->d.exp_out->count, sizeof total, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    const size_t got = (size_t)std::min<int64_t>(total, n);
    if (got > 0)
        for (int k = 0; k < 5; k++)
            if (fields & export_bits[k]) PS_HIP(c, hipMemcpyAsync(host[k], dev[k], got * export_size[k], hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    *count = total;
    return PSAMD_OK;
}

int psamd_live_stats_get(psamd_ctx *c, psamd_live_stats *out)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    if (c->wedged) return refuse_wedged(c);
    PS_HIP(c, launch_export_live(c->stream, c->P, c->d, ExportFields{nullptr, nullptr, nullptr, nullptr, nullptr}, 0,
                                 &c->d.exp_out->count, &c->d.exp_out->stats));
    PS_HIP(c, hipMemcpyAsync(out, &c->d.exp_out->stats, sizeof *out, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    return PSAMD_OK;
}

// ---- putting particles in (inject.hip) ----
static bool aligned(const void *p, size_t a) { return (uintptr_t)p % a == 0; }

// the entries' scratch for max_count entries: grows only (hipFree waits for the device; steady use never gets here)
static int inject_scratch(psamd_ctx *c, int64_t max_count)
{
    if (max_count <= c->inj_cap) return PSAMD_OK;
    for (void *p : {(void *)c->inj.ent, (void *)c->inj.tcount, (void *)c->inj.tile_out}) if (p) PS_HIP(c, hipFree(p));
    c->inj.ent = nullptr; c->inj.tcount = nullptr; c->inj.tile_out = nullptr;
    c->inj_cap = 0;
    const int64_t tiles = (max_count + INJECT_TILE - 1) / INJECT_TILE;
    PS_HIP(c, hipMalloc((void **)&c->inj.ent, (size_t)(tiles * INJECT_TILE) * sizeof(int2)));
    PS_HIP(c, hipMalloc((void **)&c->inj.tcount, (size_t)tiles * (size_t)c->geo.queue_infos * sizeof(int)));
    PS_HIP(c, hipMalloc((void **)&c->inj.tile_out, (size_t)tiles * sizeof(int)));
    c->inj_cap = tiles * INJECT_TILE;
    return PSAMD_OK;
}

int psamd_inject(psamd_ctx *c, const psamd_inject_spec *spec)
{
    if (!c || !spec) return PSAMD_ERR_INVALID_ARG;
    if (c->wedged) return refuse_wedged(c);
    if (spec->flags != 0 || spec->reserved != 0) return fail(c, PSAMD_ERR_INVALID_ARG, "inject: flags and reserved must be 0");
    if (spec->max_count < 0 || spec->max_count > INT32_MAX) return fail(c, PSAMD_ERR_INVALID_ARG, "inject: max_count outside [0, 2^31)");
    if (!spec->pos4 || !aligned(spec->pos4, 16) || !aligned(spec->vel4, 16) || !aligned(spec->fert_age, 4) || !aligned(spec->ids_dev, 4) ||
        !aligned(spec->count_dev, 8) || !aligned(spec->result_dev, 8))
        return fail(c, PSAMD_ERR_INVALID_ARG, "inject: pos4 missing, or an array misaligned");
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    PS_HIP(c, hipStreamIsCapturing(c->stream, &cs));
    if (cs != hipStreamCaptureStatusNone)
        return fail(c, PSAMD_ERR_STATE, "inject: the context's stream is being captured (the host's bound of the live count is "
                                        "kept at the call: a replay would bypass it)");
    psamd_inject_result *res = spec->result_dev ? spec->result_dev : c->inj.own;
    if (spec->max_count == 0) {
        PS_HIP(c, hipMemsetAsync(c->inj.own, 0, sizeof(psamd_inject_result), c->stream));
        if (res != c->inj.own) PS_HIP(c, hipMemsetAsync(res, 0, sizeof(psamd_inject_result), c->stream));
        return PSAMD_OK;
    }
    const int rc = inject_scratch(c, spec->max_count);
    if (rc != PSAMD_OK) return rc;
    const InjectArgs a{(const float4 *)spec->pos4, (const float4 *)spec->vel4, spec->fert_age, spec->max_count, spec->count_dev,
                       spec->ids_dev, res};
    PS_HIP(c, launch_inject(c->stream, c->P, c->S, c->d, c->geo.queue_infos, a, c->inj));
    // fill's transitions; the device's queues are ahead of the host's mirror; every entry counts in the live bound,
    // also when the record of a step enqueued before this call is read later (consume_scalars)
    c->host_queues_valid = false;
    c->grid_built = false; c->pairs_done = false; c->slab_stage = 0;
    if (c->live_bound >= 0) c->live_bound = std::min<int64_t>(c->P.slots_total, c->live_bound + spec->max_count);
    c->inject_tally[c->scalars_seq] += spec->max_count;
    return PSAMD_OK;
}

int psamd_inject_result_get(psamd_ctx *c, psamd_inject_result *out)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    if (c->wedged) return refuse_wedged(c);
    PS_HIP(c, hipMemcpyAsync(out, c->inj.own, sizeof *out, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    return PSAMD_OK;
}

// ---- taking particles out (remove.hip) ----
// the entries' scratch for max_count entries: grows only, like inject's
static int remove_scratch(psamd_ctx *c, int64_t max_count)
{
    if (max_count <= c->rem_cap) return PSAMD_OK;
    for (void *p : {(void *)c->rem.ent, (void *)c->rem.tcount, (void *)c->rem.tile_out}) if (p) PS_HIP(c, hipFree(p));
    c->rem.ent = nullptr; c->rem.tcount = nullptr; c->rem.tile_out = nullptr;
    c->rem_cap = 0;
    const int64_t tiles = (max_count + REMOVE_TILE - 1) / REMOVE_TILE;
    PS_HIP(c, hipMalloc((void **)&c->rem.ent, (size_t)(tiles * REMOVE_TILE) * sizeof(int2)));
    PS_HIP(c, hipMalloc((void **)&c->rem.tcount, (size_t)tiles * (size_t)c->geo.queue_infos * sizeof(int)));
    PS_HIP(c, hipMalloc((void **)&c->rem.tile_out, (size_t)tiles * 3 * sizeof(int)));
    c->rem_cap = tiles * REMOVE_TILE;
    return PSAMD_OK;
}

int psamd_remove(psamd_ctx *c, const psamd_remove_spec *spec)
{
    if (!c || !spec) return PSAMD_ERR_INVALID_ARG;
    if (c->wedged) return refuse_wedged(c);
    const bool box = (spec->flags & PSAMD_REMOVE_BOX) != 0;
    if ((spec->flags & ~(PSAMD_REMOVE_BOX | PSAMD_REMOVE_OUTSIDE)) || (!box && (spec->flags & PSAMD_REMOVE_OUTSIDE)) || spec->reserved != 0)
        return fail(c, PSAMD_ERR_INVALID_ARG, "remove: unknown flag bits, OUTSIDE without BOX, or reserved not 0");
    if (spec->max_count < 0 || spec->max_count > INT32_MAX) return fail(c, PSAMD_ERR_INVALID_ARG, "remove: max_count outside [0, 2^31)");
    if (!aligned(spec->ids, 4) || !aligned(spec->outcome_dev, 4) || !aligned(spec->count_dev, 8) || !aligned(spec->result_dev, 8))
        return fail(c, PSAMD_ERR_INVALID_ARG, "remove: an array misaligned");
    if (box && (spec->ids || spec->count_dev || spec->outcome_dev || spec->max_count != 0))
        return fail(c, PSAMD_ERR_INVALID_ARG, "remove: by box, ids, count_dev and outcome_dev must be NULL and max_count 0");
    if (!box && !spec->ids && spec->max_count > 0) return fail(c, PSAMD_ERR_INVALID_ARG, "remove: ids missing");
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    PS_HIP(c, hipStreamIsCapturing(c->stream, &cs));
    if (cs != hipStreamCaptureStatusNone)
        return fail(c, PSAMD_ERR_STATE, "remove: the context's stream is being captured (the call ends the host's frame in "
                                        "progress: a replay would bypass that)");
    psamd_remove_result *res = spec->result_dev ? spec->result_dev : c->rem.own;
    if (!box && spec->max_count == 0) {
        PS_HIP(c, hipMemsetAsync(c->rem.own, 0, sizeof(psamd_remove_result), c->stream));
        if (res != c->rem.own) PS_HIP(c, hipMemsetAsync(res, 0, sizeof(psamd_remove_result), c->stream));
        return PSAMD_OK;
    }
    if (box) {
        PS_HIP(c, launch_remove_box(c->stream, c->P, c->S, c->d, c->geo.queue_infos, spec->lo, spec->hi,
                                    (spec->flags & PSAMD_REMOVE_OUTSIDE) != 0, res, c->rem));
    } else {
        const int rc = remove_scratch(c, spec->max_count);
        if (rc != PSAMD_OK) return rc;
        const RemoveArgs a{spec->ids, spec->max_count, spec->count_dev, spec->outcome_dev, res};
        PS_HIP(c, launch_remove_ids(c->stream, c->P, c->S, c->d, c->geo.queue_infos, a, c->rem));
    }
    // inject's transitions; the device's queues are ahead of the host's mirror.  The host's bound of the live count stays:
    // it is an upper bound.
    c->host_queues_valid = false;
    c->grid_built = false; c->pairs_done = false; c->slab_stage = 0;
    return PSAMD_OK;
}

int psamd_remove_result_get(psamd_ctx *c, psamd_remove_result *out)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    if (c->wedged) return refuse_wedged(c);
    PS_HIP(c, hipMemcpyAsync(out, c->rem.own, sizeof *out, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    return PSAMD_OK;
}

// ---- energy (potential.hip) ----
// a frame is built, its particles have not moved, and -- a slab -- the halos are in and nothing of the plan is lent
static int potential_ready(psamd_ctx *c)
{
    if (c->wedged) return refuse_wedged(c);
    const bool ok = c->P.world > 1 ? c->slab_stage == 2 : (c->grid_built && c->slab_stage != 3);
    if (!ok) return fail(c, PSAMD_ERR_STATE, c->P.world > 1 ? "potential belongs between slab_pairs and slab_apply"
                                                             : "potential needs build_grid first, and a frame that has not been applied");
    const SlabPlan &pl = c->plan;
    if (c->P.world > 1 && (pl.lentin_lo < pl.lentin_hi || pl.lentout_lo < pl.lentout_hi))
        return fail(c, PSAMD_ERR_UNSUPPORTED, "potential: this rank's plan lends cell layers (lentin / lentout not empty); only plans "
                                              "with group-aligned cuts are served");
    return PSAMD_OK;
}

int psamd_potential(psamd_ctx *c, const psamd_potential_spec *spec)
{
    if (!c || !spec) return PSAMD_ERR_INVALID_ARG;
    if (spec->flags != 0 || spec->reserved != 0) return fail(c, PSAMD_ERR_INVALID_ARG, "potential: flags and reserved must be 0");
    if (spec->capacity < 0) return fail(c, PSAMD_ERR_INVALID_ARG, "potential: capacity < 0");
    if (!aligned(spec->phi, 4) || (!spec->phi && spec->capacity > 0) || !aligned(spec->result_dev, 8))
        return fail(c, PSAMD_ERR_INVALID_ARG, "potential: phi missing or misaligned, or result_dev misaligned");
    const int rc = potential_ready(c);
    if (rc != PSAMD_OK) return rc;
    PS_HIP(c, launch_potential(c->stream, c->P, c->d, spec->phi, spec->capacity, spec->result_dev));
    return PSAMD_OK;
}

int psamd_potential_result_get(psamd_ctx *c, psamd_potential_result *out)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    if (c->wedged) return refuse_wedged(c);
    PS_HIP(c, hipMemcpyAsync(out, &c->d.pot_out->result, sizeof *out, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    return PSAMD_OK;
}

int psamd_download_potential(psamd_ctx *c, float *phi, int64_t capacity, psamd_potential_result *out)
{
    if (!c) return PSAMD_ERR_INVALID_ARG;
    if (capacity < 0 || (!phi && capacity > 0)) return fail(c, PSAMD_ERR_INVALID_ARG, "download_potential: capacity < 0, or no array for it");
    int rc = potential_ready(c);
    if (rc != PSAMD_OK) return rc;
    const int64_t n = std::min<int64_t>(capacity, c->P.slots_total);
    rc = ensure_staging(c, std::max<size_t>((size_t)n * sizeof(float), 256));
    if (rc != PSAMD_OK) return rc;
    PS_HIP(c, launch_potential(c->stream, c->P, c->d, n > 0 ? (float *)c->staging : nullptr, n, nullptr));
    PotOut got{};
    PS_HIP(c, hipMemcpyAsync(&got, c->d.pot_out, sizeof got, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    const size_t m = (size_t)std::min<int64_t>(got.live, n);
    if (m > 0) {
        PS_HIP(c, hipMemcpyAsync(phi, c->staging, m * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        PS_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (out) *out = got.result;
    return PSAMD_OK;
}

int psamd_download_force4(psamd_ctx *c, void *out, int64_t first, int64_t count)
{
    if (!c || !out || first < 0 || count < 0 || first + count > c->P.sorted_cap) return PSAMD_ERR_INVALID_ARG;
    if (count == 0) return PSAMD_OK;
    int rc = ensure_staging(c, (size_t)count * sizeof(float4));
    if (rc != PSAMD_OK) return rc;
    PS_HIP(c, launch_force_gather(c->stream, c->P, c->d, c->staging, (int)first, (int)count));
    PS_HIP(c, hipMemcpyAsync(out, c->staging, (size_t)count * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    return PSAMD_OK;
}

// particles (pos4, vel4, acc4, cell, pflags) + QUEUE_INFO + queue, back to back
static size_t snapshot_bytes(const psamd_ctx *c)
{
    const size_t C = (size_t)c->P.slots_total;
    return C * (3 * sizeof(float4) + sizeof(int) + 1) + (size_t)c->geo.queue_infos * sizeof(QueueInfo) + C * sizeof(int);
}

static int snapshot_copy(psamd_ctx *c, bool save)
{
    const size_t C = (size_t)c->P.slots_total;
    char *p = c->snapshot;
    char *s_pos = p, *s_vel = s_pos + C * sizeof(float4), *s_acc = s_vel + C * sizeof(float4);
    char *s_cell = s_acc + C * sizeof(float4);
    char *s_qinfo = s_cell + C * sizeof(int);
    char *s_queue = s_qinfo + (size_t)c->geo.queue_infos * sizeof(QueueInfo);
    char *s_flags = s_queue + C * sizeof(int);
    if (save) {
        struct { void *dev; char *snap; size_t bytes; } parts[] = {
            {c->d.pos4, s_pos, C * sizeof(float4)}, {c->d.vel4, s_vel, C * sizeof(float4)},
            {c->d.acc4, s_acc, C * sizeof(float4)}, {c->d.cell, s_cell, C * sizeof(int)},
            {c->d.pflags, s_flags, C},
        };
        for (auto &part : parts) PS_HIP(c, hipMemcpyAsync(part.snap, part.dev, part.bytes, hipMemcpyDeviceToDevice, c->stream));
        PS_HIP(c, hipMemcpyAsync(s_qinfo, c->d.qinfo, (size_t)c->geo.queue_infos * sizeof(QueueInfo), hipMemcpyDeviceToDevice, c->stream));
        PS_HIP(c, hipMemcpyAsync(s_queue, c->d.queue, C * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
    } else {
        PS_HIP(c, launch_restore(c->stream, (int)C, s_pos, s_vel, s_acc, s_cell, s_flags, s_queue, s_qinfo,
                                 (int)((size_t)c->geo.queue_infos * sizeof(QueueInfo) / sizeof(int)), c->step, c->d));
    }
    return PSAMD_OK;
}

int psamd_snapshot_save(psamd_ctx *c)
{
    if (!c) return PSAMD_ERR_INVALID_ARG;
    if (!c->snapshot) PS_HIP(c, dev_alloc(c, &c->snapshot, snapshot_bytes(c)));
    c->snapshot_step = c->step;
    c->snapshot_live_bound = c->live_bound;
    return snapshot_copy(c, true);
}

int psamd_snapshot_restore(psamd_ctx *c)
{
    if (!c) return PSAMD_ERR_INVALID_ARG;
    if (!c->snapshot) return fail(c, PSAMD_ERR_STATE, "snapshot_restore without a saved snapshot");
    c->step = c->snapshot_step;
    c->live_bound = c->snapshot_live_bound;
    c->host_queues_valid = false;
    c->frame_reset = false; c->grid_built = false; c->pairs_done = false; c->slab_stage = 0;
    return snapshot_copy(c, false);
}

int psamd_debug_wave_trace(psamd_ctx *c, uint64_t *out, int64_t n_words)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    const int64_t have = 3 * ((int64_t)c->P.n_local_cells * c->P.slices + 4);
    PS_HIP(c, hipStreamSynchronize(c->stream));
    PS_HIP(c, hipMemcpy(out, c->d.trace, (size_t)std::min(have, n_words) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PSAMD_OK;
}

int psamd_selftest_math(psamd_ctx *c, uint32_t lo_bits, uint32_t hi_bits, uint64_t out24[24])
{
    if (!c || !out24 || hi_bits < lo_bits) return PSAMD_ERR_INVALID_ARG;
    unsigned long long *d = nullptr;
    PS_HIP(c, hipMalloc((void **)&d, 26 * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d, 0, 26 * sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) e = launch_selftest_math(c->stream, lo_bits, hi_bits, d);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out24, d, 24 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return hip_fail(c, e, "selftest_math");
    return PSAMD_OK;
}

}  // extern "C"
