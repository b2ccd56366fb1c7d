// io.hip -- state in and out of a context: fill / upload / download, snapshot, the slab message buffers, and the debug /
// self-test calls (the on-stream services -- export, inject, remove, potential -- are services.hip's).  Nothing here
// enqueues a stage of the step.
#include <random>

#include "context.hpp"

int psamd::ensure_staging(psamd_ctx *c, size_t bytes)
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
    PS_TRY(pull_queues(c));
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
        PS_TRY(ensure_staging(c, bytes));
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
    PS_TRY(push_queues(c));
    if (ids_out) std::copy(ids.begin(), ids.begin() + done, ids_out);
    if (n_done) *n_done = done;
    c->ledger.filled(placed);
    leave(c->stage, CALL_CHANGED);
    return status;
}

int psamd_upload_particles(psamd_ctx *c, const void *p72, int64_t first, int64_t count)
{
    if (!c || !p72 || first < 0 || count < 0 || first + count > c->geo.container) return PSAMD_ERR_INVALID_ARG;
    if (count == 0) return PSAMD_OK;
    PS_TRY(ensure_staging(c, (size_t)count * 72));
    PS_HIP(c, hipMemcpyAsync(c->staging, p72, (size_t)count * 72, hipMemcpyHostToDevice, c->stream));
    // odd grids are not centred (G/2 is an integer division): allow the longer half
    const float half_box = (float)((c->geo.G - c->geo.G / 2) * c->geo.cfg.cell_size);
    PS_HIP(c, launch_unpack_aos(c->stream, c->P, c->staging, (int)first, (int)count, half_box, c->d));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    leave(c->stage, CALL_CHANGED);
    c->ledger.uploaded();
    return check_device_errors(c);
}

int psamd_download_particles(psamd_ctx *c, void *p72, int64_t first, int64_t count)
{
    if (!c || !p72 || first < 0 || count < 0 || first + count > c->geo.container) return PSAMD_ERR_INVALID_ARG;
    if (count == 0) return PSAMD_OK;
    PS_TRY(ensure_staging(c, (size_t)count * 72));
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
    PS_TRY(pull_queues(c));
    std::memcpy(qi, c->h_qinfo.data(), c->h_qinfo.size() * sizeof(QueueInfo));
    std::memcpy(queue, c->h_queue.data(), c->h_queue.size() * sizeof(int32_t));
    return PSAMD_OK;
}

// Rebuild the reference's fixed-stride lists from the compact sorted arrays.  start[] is
// indexed by the own LOCAL cells (region 0); local cell lc is global cell lc + cell_off.
static int fetch_sorted(psamd_ctx *c, std::vector<int> &start, std::vector<int> &ids)
{
    if (!built(c->stage)) return fail(c, PSAMD_ERR_STATE, "grid lists requested before build_grid");
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
    PS_TRY(fetch_sorted(c, start, ids));
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
    if (!pairs_done(c->stage)) return fail(c, PSAMD_ERR_STATE, "force counts requested before the pair pass of this frame");
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

// n cells from `first` of `count` moment planes from plane `plane0` on, cell by cell: float4 = (X, Y, Z, M) of the four
// first planes, float[6] = (Cxx, Cyy, Czz, Cxy, Cxz, Cyz) of the six behind them; waits for the stream
static int download_moments(psamd_ctx *c, size_t first, size_t n, float *o, size_t plane0 = 0, size_t count = 4)
{
    const size_t cap = (size_t)c->d.mom_cap;
    std::vector<float> planes(count * n);
    for (size_t f = 0; f < count; f++)
        PS_HIP(c, hipMemcpyAsync(planes.data() + f * n, c->d.cell_mom + (plane0 + f) * cap + first, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < n; k++)
        for (size_t f = 0; f < count; f++) o[count * k + f] = planes[f * n + k];
    return PSAMD_OK;
}

int psamd_download_cell_moments(psamd_ctx *c, void *out)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    if (!(c->P.flags & (PSAMD_FLAG_FAR_MONOPOLE | PSAMD_FLAG_FAR_PYRAMID))) return fail(c, PSAMD_ERR_UNSUPPORTED, "cell moments are formed on a context with far monopoles (PSAMD_FLAG_FAR_MONOPOLE, PSAMD_FLAG_FAR_PYRAMID) only");
    if (!pairs_done(c->stage)) return fail(c, PSAMD_ERR_STATE, "cell moments requested before the pair pass of this frame");
    return download_moments(c, 0, (size_t)c->geo.num_cells, static_cast<float *>(out));      // (a pyramid's level 0 starts the planes)
}

int psamd_far_levels(const psamd_config *cfg, int32_t *levels, int32_t dims[16])
{
    if (!cfg || !levels || !dims) return PSAMD_ERR_INVALID_ARG;
    Geometry g;
    if (!g.init(*cfg)) return PSAMD_ERR_INVALID_ARG;
    const FarLevels lev = far_levels_of(g.G);
    *levels = lev.n;
    for (int k = 0; k < 16; k++) dims[k] = k < lev.n ? lev.G[k] : 0;
    return PSAMD_OK;
}

int psamd_download_level_moments(psamd_ctx *c, int32_t level, void *out)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    if (!(c->P.flags & PSAMD_FLAG_FAR_PYRAMID)) return fail(c, PSAMD_ERR_UNSUPPORTED, "level moments are formed on a context with the pyramid of monopoles (PSAMD_FLAG_FAR_PYRAMID) only");
    const FarLevels &lev = c->d.lev;
    if (level < 0 || level >= lev.n) return fail(c, PSAMD_ERR_INVALID_ARG, "level moments: no such level");
    if (!pairs_done(c->stage)) return fail(c, PSAMD_ERR_STATE, "level moments requested before the pair pass of this frame");
    const size_t G = (size_t)lev.G[level];
    return download_moments(c, (size_t)lev.off[level], G * G * G, static_cast<float *>(out));
}

int psamd_download_level_quadrupoles(psamd_ctx *c, int32_t level, void *out)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    if (!(c->P.flags & PSAMD_FLAG_FAR_QUADRUPOLE)) return fail(c, PSAMD_ERR_UNSUPPORTED, "level quadrupoles are formed on a context with quadrupoles on the pyramid (PSAMD_FLAG_FAR_QUADRUPOLE) only");
    const FarLevels &lev = c->d.lev;
    if (level < 0 || level >= lev.n) return fail(c, PSAMD_ERR_INVALID_ARG, "level quadrupoles: no such level");
    if (!pairs_done(c->stage)) return fail(c, PSAMD_ERR_STATE, "level quadrupoles requested before the pair pass of this frame");
    const size_t G = (size_t)lev.G[level];
    return download_moments(c, (size_t)lev.off[level], G * G * G, static_cast<float *>(out), 4, 6);
}

int psamd_download_chunkgrid(psamd_ctx *c, int32_t *out)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    std::vector<int> start, ids;
    PS_TRY(fetch_sorted(c, start, ids));
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
    if (rc != PSAMD_OK && !built(c->stage)) return rc;
    if (built(c->stage)) {
        FrameScalars fs{};
        PS_HIP(c, hipMemcpy(&fs, c->d.fs, sizeof fs, hipMemcpyDeviceToHost));
        out2[0] = fs.gridmax[0]; out2[1] = fs.gridmax[1];
        c->ledger.frame_live(fs.live);
    } else { out2[0] = c->ledger.last().gridmax[0]; out2[1] = c->ledger.last().gridmax[1]; }
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
    o->particles_processed = c->ledger.particles_processed();
    o->max_ops_one_queue = c->ledger.longest_list();
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
    o->live = c->ledger.last_live();
    o->stream = (void *)c->stream;
    return PSAMD_OK;
}

int psamd_download_force4(psamd_ctx *c, void *out, int64_t first, int64_t count)
{
    if (!c || !out || first < 0 || count < 0 || first + count > c->P.sorted_cap) return PSAMD_ERR_INVALID_ARG;
    if (count == 0) return PSAMD_OK;
    PS_TRY(ensure_staging(c, (size_t)count * sizeof(float4)));
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
    c->ledger.snapshot_saved();
    return snapshot_copy(c, true);
}

int psamd_snapshot_restore(psamd_ctx *c)
{
    if (!c) return PSAMD_ERR_INVALID_ARG;
    if (!c->snapshot) return fail(c, PSAMD_ERR_STATE, "snapshot_restore without a saved snapshot");
    c->step = c->snapshot_step;
    c->ledger.snapshot_restored();
    end_frame(c, CALL_RESTORE);
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

int psamd_debug_packs(psamd_ctx *c, int32_t *cells, int64_t capacity, int64_t *count, uint64_t *shape)
{
    if (!c || !count || capacity < 0 || (capacity > 0 && !cells)) return PSAMD_ERR_INVALID_ARG;
    FrameScalars fs;
    PS_HIP(c, hipStreamSynchronize(c->stream));
    PS_HIP(c, hipMemcpy(&fs, c->d.fs, sizeof fs, hipMemcpyDeviceToHost));
    // (only the two-pass stage runs the plan that writes n_merged: any other launch shape has no packs, whatever the word holds)
    const bool planned = (c->pairs_shape_last >> 11 & 1) != 0;
    const int64_t have = planned ? std::max<int64_t>(0, std::min<int64_t>(fs.n_merged, c->P.n_local_cells)) : 0;
    *count = have;
    if (shape) *shape = c->pairs_shape_last;
    const int64_t n = std::min(have, capacity);
    if (n > 0) PS_HIP(c, hipMemcpy(cells, c->d.merged_tasks, (size_t)n * sizeof(int4), hipMemcpyDeviceToHost));
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
