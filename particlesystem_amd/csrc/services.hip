// services.hip -- the host side of the on-stream services: psamd_export_live (export.hip), psamd_inject (inject.hip),
// psamd_remove (remove.hip), psamd_update (update.hip), psamd_potential (potential.hip), psamd_probe (probe.hip), psamd_deposit (deposit.hip), psamd_sample (sample.hip), psamd_neighbours (neighbours.hip), psamd_groups (groups.hip), psamd_knn (knn.hip), their host-array forms and their result records.
// A service enqueues its launches on the context's stream and returns; nothing here enqueues a stage of the step.
#include "context.hpp"

#include <cmath>

// ---- what the services share ----
static bool aligned(const void *p, size_t a) { return (uintptr_t)p % a == 0; }

// the prelude of a call that needs a live context and its one mandatory argument
static int service_args(psamd_ctx *c, const void *arg)
{
    if (!c || !arg) return PSAMD_ERR_INVALID_ARG;
    return c->wedged ? refuse_wedged(c) : PSAMD_OK;
}

// a call that changes the host's view of the frame cannot be replayed from a captured graph
static int refuse_capture(psamd_ctx *c, const char *who, const char *why)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    PS_HIP(c, hipStreamIsCapturing(c->stream, &cs));
    if (cs == hipStreamCaptureStatusNone) return PSAMD_OK;
    return fail(c, PSAMD_ERR_STATE, std::string(who) + ": the context's stream is being captured (" + why + ")");
}

// a call with nothing to do: the context's own result record and the caller's, zeroed on the stream
static int zero_result(psamd_ctx *c, void *own, void *res, size_t bytes)
{
    PS_HIP(c, hipMemsetAsync(own, 0, bytes, c->stream));
    if (res != own) PS_HIP(c, hipMemsetAsync(res, 0, bytes, c->stream));
    return PSAMD_OK;
}

// a *_result_get: the context's own record, once the stream has reached it
static int read_own(psamd_ctx *c, void *out, const void *src, size_t bytes)
{
    PS_TRY(service_args(c, out));
    PS_HIP(c, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    return PSAMD_OK;
}

// The slots or the queues changed on the device: the host's frame in progress is over and its queue mirror is behind.
void psamd::end_frame(psamd_ctx *c, Call why)
{
    c->host_queues_valid = false;
    leave(c->stage, why);
}

// the entries' scratch for max_count entries: grows only (hipFree waits for the device; steady use never gets here)
static int grow_entry_scratch(psamd_ctx *c, EntryScratch &s, int64_t max_count, int tile_out_words)
{
    if (max_count <= s.cap) return PSAMD_OK;
    for (void *p : {(void *)s.ent, (void *)s.tcount, (void *)s.tile_out}) if (p) PS_HIP(c, hipFree(p));
    s = EntryScratch{};
    const int64_t tiles = (max_count + ENTRY_TILE - 1) / ENTRY_TILE;
    PS_HIP(c, hipMalloc((void **)&s.ent, (size_t)(tiles * ENTRY_TILE) * sizeof(int2)));
    PS_HIP(c, hipMalloc((void **)&s.tcount, (size_t)tiles * (size_t)c->geo.queue_infos * sizeof(int)));
    PS_HIP(c, hipMalloc((void **)&s.tile_out, (size_t)tiles * tile_out_words * sizeof(int)));
    s.cap = tiles * ENTRY_TILE;
    return PSAMD_OK;
}

extern "C" {

// ---- getting frames out (export.hip) ----
static const uint32_t export_bits[5] = {PSAMD_EXPORT_POS, PSAMD_EXPORT_VEL, PSAMD_EXPORT_ACC, PSAMD_EXPORT_ID, PSAMD_EXPORT_CELL};
static const size_t export_size[5] = {sizeof(float4), sizeof(float4), sizeof(float4), sizeof(int32_t), sizeof(int32_t)};

// device: the kernel stores to the arrays (float4 and int32 stores want their natural alignment); host arrays are copied into
static int export_args(psamd_ctx *c, uint32_t fields, void *const ptr[5], int64_t capacity, bool device)
{
    if (fields & ~PSAMD_EXPORT_ALL) return fail(c, PSAMD_ERR_INVALID_ARG, "export: unknown field bits");
    if (capacity < 0) return fail(c, PSAMD_ERR_INVALID_ARG, "export: capacity < 0");
    for (int k = 0; k < 5; k++)
        if ((fields & export_bits[k]) && (!ptr[k] || (device && !aligned(ptr[k], export_size[k]))))
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
    PS_TRY(service_args(c, spec));
    void *const ptr[5] = {spec->pos4, spec->vel4, spec->acc4, spec->id, spec->cell};
    if (spec->reserved != 0) return fail(c, PSAMD_ERR_INVALID_ARG, "export: reserved must be 0");
    PS_TRY(export_args(c, spec->fields, ptr, spec->capacity, true));
    PS_HIP(c, launch_export_live(c->stream, c->P, c->d, export_fields(spec->fields, ptr), spec->capacity,
                                 spec->count_dev ? spec->count_dev : &c->d.exp_out->count,
                                 spec->stats_dev ? spec->stats_dev : &c->d.exp_out->stats));
    return PSAMD_OK;
}

int psamd_download_live(psamd_ctx *c, uint32_t fields, void *pos4, void *vel4, void *acc4, int32_t *id, int32_t *cell,
                        int64_t capacity, int64_t *count)
{
    PS_TRY(service_args(c, count));
    void *const host[5] = {pos4, vel4, acc4, id, cell};
    PS_TRY(export_args(c, fields, host, capacity, false));
    // the chosen fields of at most min(capacity, owned slots) particles, one after the other in the staging buffer
    const int64_t n = std::min<int64_t>(capacity, c->P.slots_total);
    size_t off[5] = {0, 0, 0, 0, 0}, bytes = 0;
    for (int k = 0; k < 5; k++)
        if (fields & export_bits[k]) { off[k] = bytes; bytes += ((size_t)n * export_size[k] + 255) / 256 * 256; }
    PS_TRY(ensure_staging(c, std::max<size_t>(bytes, 256)));
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
    PS_TRY(service_args(c, out));
    PS_HIP(c, launch_export_live(c->stream, c->P, c->d, ExportFields{nullptr, nullptr, nullptr, nullptr, nullptr}, 0,
                                 &c->d.exp_out->count, &c->d.exp_out->stats));
    PS_HIP(c, hipMemcpyAsync(out, &c->d.exp_out->stats, sizeof *out, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    return PSAMD_OK;
}

// ---- putting particles in (inject.hip) ----
int psamd_inject(psamd_ctx *c, const psamd_inject_spec *spec)
{
    PS_TRY(service_args(c, spec));
    if (spec->flags != 0 || spec->reserved != 0) return fail(c, PSAMD_ERR_INVALID_ARG, "inject: flags and reserved must be 0");
    if (spec->max_count < 0 || spec->max_count > INT32_MAX) return fail(c, PSAMD_ERR_INVALID_ARG, "inject: max_count outside [0, 2^31)");
    if (!spec->pos4 || !aligned(spec->pos4, 16) || !aligned(spec->vel4, 16) || !aligned(spec->fert_age, 4) || !aligned(spec->ids_dev, 4) ||
        !aligned(spec->count_dev, 8) || !aligned(spec->result_dev, 8))
        return fail(c, PSAMD_ERR_INVALID_ARG, "inject: pos4 missing, or an array misaligned");
    PS_TRY(refuse_capture(c, "inject", "the host's bound of the live count is kept at the call: a replay would bypass it"));
    psamd_inject_result *res = spec->result_dev ? spec->result_dev : c->inj.own;
    if (spec->max_count == 0) return zero_result(c, c->inj.own, res, sizeof *res);
    PS_TRY(grow_entry_scratch(c, c->inj.e, spec->max_count, 1));
    const InjectArgs a{(const float4 *)spec->pos4, (const float4 *)spec->vel4, spec->fert_age, spec->max_count, spec->count_dev,
                       spec->ids_dev, res};
    PS_HIP(c, launch_inject(c->stream, c->P, c->S, c->d, c->geo.queue_infos, a, c->inj));
    // fill's transitions, and the device's queues are ahead of the host's mirror; every entry counts in the live bound
    end_frame(c);
    c->ledger.injected(ledger_params(c), spec->max_count);
    return PSAMD_OK;
}

int psamd_inject_result_get(psamd_ctx *c, psamd_inject_result *out) { return read_own(c, out, c ? c->inj.own : nullptr, sizeof *out); }

// ---- taking particles out (remove.hip) ----
int psamd_remove(psamd_ctx *c, const psamd_remove_spec *spec)
{
    PS_TRY(service_args(c, spec));
    const bool box = (spec->flags & PSAMD_REMOVE_BOX) != 0;
    if ((spec->flags & ~(PSAMD_REMOVE_BOX | PSAMD_REMOVE_OUTSIDE)) || (!box && (spec->flags & PSAMD_REMOVE_OUTSIDE)) || spec->reserved != 0)
        return fail(c, PSAMD_ERR_INVALID_ARG, "remove: unknown flag bits, OUTSIDE without BOX, or reserved not 0");
    if (spec->max_count < 0 || spec->max_count > INT32_MAX) return fail(c, PSAMD_ERR_INVALID_ARG, "remove: max_count outside [0, 2^31)");
    if (!aligned(spec->ids, 4) || !aligned(spec->outcome_dev, 4) || !aligned(spec->count_dev, 8) || !aligned(spec->result_dev, 8))
        return fail(c, PSAMD_ERR_INVALID_ARG, "remove: an array misaligned");
    if (box && (spec->ids || spec->count_dev || spec->outcome_dev || spec->max_count != 0))
        return fail(c, PSAMD_ERR_INVALID_ARG, "remove: by box, ids, count_dev and outcome_dev must be NULL and max_count 0");
    if (!box && !spec->ids && spec->max_count > 0) return fail(c, PSAMD_ERR_INVALID_ARG, "remove: ids missing");
    PS_TRY(refuse_capture(c, "remove", "the call ends the host's frame in progress: a replay would bypass that"));
    psamd_remove_result *res = spec->result_dev ? spec->result_dev : c->rem.own;
    if (!box && spec->max_count == 0) return zero_result(c, c->rem.own, res, sizeof *res);
    if (box) {
        PS_HIP(c, launch_remove_box(c->stream, c->P, c->S, c->d, c->geo.queue_infos, spec->lo, spec->hi,
                                    (spec->flags & PSAMD_REMOVE_OUTSIDE) != 0, res, c->rem));
    } else {
        PS_TRY(grow_entry_scratch(c, c->rem.e, spec->max_count, 3));
        const RemoveArgs a{spec->ids, spec->max_count, spec->count_dev, spec->outcome_dev, res};
        PS_HIP(c, launch_remove_ids(c->stream, c->P, c->S, c->d, c->geo.queue_infos, a, c->rem));
    }
    // The host's bound of the live count stays: it is an upper bound.
    end_frame(c);
    return PSAMD_OK;
}

int psamd_remove_result_get(psamd_ctx *c, psamd_remove_result *out) { return read_own(c, out, c ? c->rem.own : nullptr, sizeof *out); }

// ---- changing particles in place (update.hip) ----
// the entries' codes for max_count entries: grows only, and not under a capture (grow_probe_scratch's rule)
static int grow_update_scratch(psamd_ctx *c, UpdateScratch &s, int64_t max_count)
{
    if (max_count <= s.cap) return PSAMD_OK;
    PS_TRY(refuse_capture(c, "update", "max_count exceeds every earlier call's: the scratch would have to grow"));
    if (s.code) PS_HIP(c, hipFree(s.code));
    s.code = nullptr; s.cap = 0;
    const int64_t room = (max_count + ENTRY_TILE - 1) / ENTRY_TILE * ENTRY_TILE;
    PS_HIP(c, hipMalloc((void **)&s.code, (size_t)room * sizeof(int)));
    s.cap = room;
    return PSAMD_OK;
}

int psamd_update(psamd_ctx *c, const psamd_update_spec *spec)
{
    PS_TRY(service_args(c, spec));
    const uint32_t words = PSAMD_UPDATE_VEL | PSAMD_UPDATE_AGE | PSAMD_UPDATE_MASS | PSAMD_UPDATE_FERT, f = spec->fields;
    const bool order = (f & PSAMD_UPDATE_EXPORT_ORDER) != 0, some = spec->max_count > 0;
    if ((f & words) == 0 || (f & ~(words | PSAMD_UPDATE_ADD | PSAMD_UPDATE_EXPORT_ORDER)) || ((f & PSAMD_UPDATE_ADD) && !(f & PSAMD_UPDATE_VEL)) ||
        spec->reserved != 0)
        return fail(c, PSAMD_ERR_INVALID_ARG, "update: no field bit, unknown bits, ADD without VEL, or reserved not 0");
    if (spec->max_count < 0 || spec->max_count > INT32_MAX) return fail(c, PSAMD_ERR_INVALID_ARG, "update: max_count outside [0, 2^31)");
    if (!aligned(spec->ids, 4) || !aligned(spec->vel4, 16) || !aligned(spec->w, 4) || !aligned(spec->fert_age, 4) ||
        !aligned(spec->outcome_dev, 4) || !aligned(spec->count_dev, 8) || !aligned(spec->result_dev, 8))
        return fail(c, PSAMD_ERR_INVALID_ARG, "update: an array misaligned");
    if (order ? spec->ids != nullptr : some && !spec->ids)
        return fail(c, PSAMD_ERR_INVALID_ARG, "update: ids missing, or given with PSAMD_UPDATE_EXPORT_ORDER");
    if (some && (((f & (PSAMD_UPDATE_VEL | PSAMD_UPDATE_AGE)) && !spec->vel4) || ((f & PSAMD_UPDATE_MASS) && !spec->w) ||
                 ((f & PSAMD_UPDATE_FERT) && !spec->fert_age)))
        return fail(c, PSAMD_ERR_INVALID_ARG, "update: an array the fields name is missing");
    if (!update_window(c->stage))
        return fail(c, PSAMD_ERR_STATE, "update: between slab_apply and slab_finish the departing particles are staged (an update of the "
                                        "slots they leave would be lost)");
    // the snapshot holds w_eff and age: a new mass or age ends the frame in progress, velocity and fertility age do not
    const bool ends = (f & (PSAMD_UPDATE_MASS | PSAMD_UPDATE_AGE)) != 0;
    if (ends) PS_TRY(refuse_capture(c, "update", "a new mass or age ends the host's frame in progress: a replay would bypass that"));
    psamd_update_result *res = spec->result_dev ? spec->result_dev : c->upd.own;
    if (!some) return zero_result(c, c->upd.own, res, sizeof *res);
    const UpdateArgs a{f, spec->ids, (const float4 *)spec->vel4, spec->w, spec->fert_age, spec->max_count, spec->count_dev, spec->outcome_dev, res};
    if (order) PS_HIP(c, launch_update_order(c->stream, c->P, c->d, a, c->upd));
    else {
        PS_TRY(grow_update_scratch(c, c->upd, spec->max_count));
        PS_HIP(c, launch_update_ids(c->stream, c->P, c->d, a, c->upd, c->rem.claim));
    }
    if (ends) end_frame(c);
    return PSAMD_OK;
}

int psamd_update_result_get(psamd_ctx *c, psamd_update_result *out) { return read_own(c, out, c ? c->upd.own : nullptr, sizeof *out); }

// ---- energy (potential.hip) ----
// a frame is built, its particles have not moved, and -- a slab -- the halos are in (potential and probe)
static int frame_ready(psamd_ctx *c, const char *who)
{
    if (c->wedged) return refuse_wedged(c);
    if (!field_window(c->stage, c->P.world)) return fail(c, PSAMD_ERR_STATE, std::string(who) + (c->P.world > 1 ? " belongs between slab_pairs and slab_apply"
                                                                                : " needs build_grid first, and a frame that has not been applied"));
    return PSAMD_OK;
}

static bool quad_context(const psamd_ctx *c) { return (c->P.flags & PSAMD_FLAG_FAR_QUADRUPOLE) != 0; }

// the modifier bits this context kind knows: the far form on far-monopole contexts, its quadrupole form on quadrupole contexts
static uint32_t potential_bits(const psamd_ctx *c)
{
    return (far_context(c->P.flags) ? PSAMD_POTENTIAL_FAR : 0u) | (quad_context(c) ? PSAMD_POTENTIAL_QUADRUPOLE : 0u);
}

static uint32_t probe_far_bits(const psamd_ctx *c)
{
    return (far_context(c->P.flags) ? PSAMD_PROBE_FAR : 0u) | (quad_context(c) ? PSAMD_PROBE_QUADRUPOLE : 0u);
}

// potential and probe promise exactly the bodies the force pass walks: with far monopoles (flat or as a pyramid) a
// stencil-only answer would break that silently, and a caller written for the stencil's bodies is never handed another
// quantity -- the monopole form is served only where it is asked for (PSAMD_POTENTIAL_FAR, PSAMD_PROBE_FAR)
// ... and on a quadrupole context (PSAMD_FLAG_FAR_QUADRUPOLE) the far form alone is monopoles only, not that context's field
// either: there the quadrupole form is served, where both bits ask for it (PSAMD_POTENTIAL_QUADRUPOLE, PSAMD_PROBE_QUADRUPOLE)
static int refuse_far_monopole(psamd_ctx *c, const char *who, bool far_asked, bool quad_asked)
{
    if (quad_context(c) && !(far_asked && quad_asked))
        return fail(c, PSAMD_ERR_UNSUPPORTED, std::string(who) + ": on a context with quadrupoles on the pyramid (PSAMD_FLAG_FAR_QUADRUPOLE) only the "
                                              "quadrupole far form is served (PSAMD_POTENTIAL_FAR | PSAMD_POTENTIAL_QUADRUPOLE, "
                                              "PSAMD_PROBE_FAR | PSAMD_PROBE_QUADRUPOLE); the far form alone is monopoles only");
    if (far_context(c->P.flags) && !far_asked)
        return fail(c, PSAMD_ERR_UNSUPPORTED, std::string(who) + ": on a context with far monopoles (PSAMD_FLAG_FAR_MONOPOLE, PSAMD_FLAG_FAR_PYRAMID) "
                                              "only the far form is served (PSAMD_POTENTIAL_FAR, psamd_download_potential_far, PSAMD_PROBE_FAR)");
    return PSAMD_OK;
}

// the far field on slabs (PSAMD_FLAG_FAR_SLAB, world > 1) serves the step alone: the far forms of potential and probe there
// need the lent layers' and the window's rules worked out, and the stencil-only forms are not this context's field
static int refuse_far_slab(psamd_ctx *c, const char *who)
{
    if (far_context(c->P.flags) && c->P.world > 1)
        return fail(c, PSAMD_ERR_UNSUPPORTED, std::string(who) + ": a far-field context on slabs (PSAMD_FLAG_FAR_SLAB, world > 1) serves the step only");
    return PSAMD_OK;
}

// ... and nothing of the plan is lent (potential and neighbours)
static int window_nothing_lent(psamd_ctx *c, const char *who)
{
    PS_TRY(frame_ready(c, who));
    const SlabPlan &pl = c->plan;
    if (c->P.world > 1 && (pl.lentin_lo < pl.lentin_hi || pl.lentout_lo < pl.lentout_hi))
        return fail(c, PSAMD_ERR_UNSUPPORTED, std::string(who) + ": this rank's plan lends cell layers (lentin / lentout not empty); only plans "
                                              "with group-aligned cuts are served");
    return PSAMD_OK;
}

static int potential_ready(psamd_ctx *c, uint32_t flags)
{
    PS_TRY(refuse_far_monopole(c, "potential", (flags & PSAMD_POTENTIAL_FAR) != 0, (flags & PSAMD_POTENTIAL_QUADRUPOLE) != 0));
    return window_nothing_lent(c, "potential");
}

// the spec's flags, of psamd_potential and of its host forms: no bit this context kind does not know, no modifier alone
static int potential_flags(psamd_ctx *c, uint32_t flags)
{
    if (flags & ~potential_bits(c))
        return fail(c, PSAMD_ERR_INVALID_ARG, "potential: unknown flag bits (PSAMD_POTENTIAL_FAR belongs to far-monopole contexts, "
                                              "PSAMD_POTENTIAL_QUADRUPOLE to quadrupole contexts)");
    if ((flags & PSAMD_POTENTIAL_QUADRUPOLE) && !(flags & PSAMD_POTENTIAL_FAR))
        return fail(c, PSAMD_ERR_INVALID_ARG, "potential: PSAMD_POTENTIAL_QUADRUPOLE is a modifier of PSAMD_POTENTIAL_FAR");
    return PSAMD_OK;
}

int psamd_potential(psamd_ctx *c, const psamd_potential_spec *spec)
{
    if (!c || !spec) return PSAMD_ERR_INVALID_ARG;
    PS_TRY(refuse_far_slab(c, "potential"));
    PS_TRY(potential_flags(c, spec->flags));
    if (spec->reserved != 0) return fail(c, PSAMD_ERR_INVALID_ARG, "potential: reserved not 0");
    if (spec->capacity < 0) return fail(c, PSAMD_ERR_INVALID_ARG, "potential: capacity < 0");
    if (!aligned(spec->phi, 4) || (!spec->phi && spec->capacity > 0) || !aligned(spec->result_dev, 8))
        return fail(c, PSAMD_ERR_INVALID_ARG, "potential: phi missing or misaligned, or result_dev misaligned");
    PS_TRY(potential_ready(c, spec->flags));
    PS_HIP(c, launch_potential(c->stream, c->P, c->d, spec->phi, spec->capacity, spec->result_dev, spec->flags));
    return PSAMD_OK;
}

int psamd_potential_result_get(psamd_ctx *c, psamd_potential_result *out) { return read_own(c, out, c ? &c->d.pot_out->result : nullptr, sizeof *out); }

// the one body of psamd_download_potential, psamd_download_potential_far and psamd_download_potential_flags; `checked`: the
// flags are a caller's and are validated as psamd_potential validates them (the two old forms keep their statuses: on a
// context without far monopoles the far form is PSAMD_ERR_UNSUPPORTED, behind the argument checks)
static int download_potential(psamd_ctx *c, uint32_t flags, bool checked, float *phi, int64_t capacity, psamd_potential_result *out)
{
    if (!c) return PSAMD_ERR_INVALID_ARG;
    PS_TRY(refuse_far_slab(c, "download_potential"));
    if (checked) PS_TRY(potential_flags(c, flags));
    if (capacity < 0 || (!phi && capacity > 0)) return fail(c, PSAMD_ERR_INVALID_ARG, "download_potential: capacity < 0, or no array for it");
    if (!checked && (flags & PSAMD_POTENTIAL_FAR) && !far_context(c->P.flags))
        return fail(c, PSAMD_ERR_UNSUPPORTED, "download_potential_far: the context has no far monopoles (PSAMD_FLAG_FAR_MONOPOLE, PSAMD_FLAG_FAR_PYRAMID)");
    PS_TRY(potential_ready(c, flags));
    const int64_t n = std::min<int64_t>(capacity, c->P.slots_total);
    PS_TRY(ensure_staging(c, std::max<size_t>((size_t)n * sizeof(float), 256)));
    PS_HIP(c, launch_potential(c->stream, c->P, c->d, n > 0 ? (float *)c->staging : nullptr, n, nullptr, flags));
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

int psamd_download_potential(psamd_ctx *c, float *phi, int64_t capacity, psamd_potential_result *out)
{
    return download_potential(c, 0u, false, phi, capacity, out);
}

int psamd_download_potential_far(psamd_ctx *c, float *phi, int64_t capacity, psamd_potential_result *out)
{
    return download_potential(c, PSAMD_POTENTIAL_FAR, false, phi, capacity, out);
}

int psamd_download_potential_flags(psamd_ctx *c, uint32_t flags, float *phi, int64_t capacity, psamd_potential_result *out)
{
    return download_potential(c, flags, true, phi, capacity, out);
}

// ---- the field at chosen points (probe.hip) ----
// the probes' scratch for max_count entries: grows only, and not under a capture (hipFree / hipMalloc cannot be recorded)
static int grow_probe_scratch(psamd_ctx *c, ProbeScratch &s, int64_t max_count)
{
    if (max_count <= s.cap) return PSAMD_OK;
    PS_TRY(refuse_capture(c, "probe", "max_count exceeds every earlier call's: the scratch would have to grow"));
    for (void *p : {(void *)s.code, (void *)s.order}) if (p) PS_HIP(c, hipFree(p));
    s.code = s.order = nullptr; s.cap = 0;
    const int64_t room = (max_count + ENTRY_TILE - 1) / ENTRY_TILE * ENTRY_TILE;
    PS_HIP(c, hipMalloc((void **)&s.code, (size_t)room * sizeof(int)));
    PS_HIP(c, hipMalloc((void **)&s.order, (size_t)room * sizeof(int)));
    s.cap = room;
    return PSAMD_OK;
}

int psamd_probe(psamd_ctx *c, const psamd_probe_spec *spec)
{
    PS_TRY(service_args(c, spec));
    PS_TRY(refuse_far_slab(c, "probe"));
    // (PSAMD_PROBE_FAR is a known bit on far-monopole contexts only, PSAMD_PROBE_QUADRUPOLE on quadrupole contexts only, and both
    // are modifiers: they ask for no component)
    if ((spec->fields & (PSAMD_PROBE_ACC | PSAMD_PROBE_PHI)) == 0 ||
        (spec->fields & ~(PSAMD_PROBE_ACC | PSAMD_PROBE_PHI | probe_far_bits(c))) || spec->reserved != 0)
        return fail(c, PSAMD_ERR_INVALID_ARG, "probe: fields without PSAMD_PROBE_ACC or PSAMD_PROBE_PHI or with unknown bits (PSAMD_PROBE_FAR belongs "
                                              "to far-monopole contexts, PSAMD_PROBE_QUADRUPOLE to quadrupole contexts), or reserved not 0");
    if ((spec->fields & PSAMD_PROBE_QUADRUPOLE) && !(spec->fields & PSAMD_PROBE_FAR))
        return fail(c, PSAMD_ERR_INVALID_ARG, "probe: PSAMD_PROBE_QUADRUPOLE is a modifier of PSAMD_PROBE_FAR");
    if (spec->max_count < 0 || spec->max_count > INT32_MAX) return fail(c, PSAMD_ERR_INVALID_ARG, "probe: max_count outside [0, 2^31)");
    if ((spec->max_count > 0 && (!spec->pos4 || !spec->out4)) || !aligned(spec->pos4, 16) || !aligned(spec->out4, 16) ||
        !aligned(spec->outcome_dev, 4) || !aligned(spec->count_dev, 8) || !aligned(spec->result_dev, 8))
        return fail(c, PSAMD_ERR_INVALID_ARG, "probe: pos4 or out4 missing, or an array misaligned");
    if ((c->P.flags & PSAMD_FLAG_ALL_PAIRS) && c->P.world > 1)
        return fail(c, PSAMD_ERR_UNSUPPORTED, "probe: all-pairs contexts are served on one context only (world == 1)");
    PS_TRY(refuse_far_monopole(c, "probe", (spec->fields & PSAMD_PROBE_FAR) != 0, (spec->fields & PSAMD_PROBE_QUADRUPOLE) != 0));
    PS_TRY(frame_ready(c, "probe"));
    psamd_probe_result *res = spec->result_dev ? spec->result_dev : c->prb.own;
    if (spec->max_count == 0) return zero_result(c, c->prb.own, res, sizeof *res);
    PS_TRY(grow_probe_scratch(c, c->prb, spec->max_count));
    const ProbeArgs a{spec->fields, (const float4 *)spec->pos4, spec->max_count, spec->count_dev, (float4 *)spec->out4, spec->outcome_dev, res};
    PS_HIP(c, launch_probe(c->stream, c->P, c->d, a, c->prb));
    return PSAMD_OK;
}

int psamd_probe_result_get(psamd_ctx *c, psamd_probe_result *out) { return read_own(c, out, c ? c->prb.own : nullptr, sizeof *out); }

// ---- mass on a lattice (deposit.hip) ----
// the lattice of refine k on this context's grid, or nothing (refine not 1, 2 or 4)
static bool deposit_lattice(const psamd_ctx *c, int32_t refine, DepLattice &a, int64_t &voxels)
{
    if (refine != 1 && refine != 2 && refine != 4) return false;
    const int G = c->P.G;
    a.refine = refine; a.M = G * refine;
    a.inv_h = (float)((double)refine / c->P.cell_size);
    a.off = (float)((G / 2) * refine) - 0.5f;
    a.top = (float)(a.M - 1);
    voxels = (int64_t)a.M * a.M * a.M;
    return true;
}

int psamd_deposit(psamd_ctx *c, const psamd_deposit_spec *spec)
{
    PS_TRY(service_args(c, spec));
    DepositArgs a{};
    int64_t voxels = 0;
    if (spec->flags != 0) return fail(c, PSAMD_ERR_INVALID_ARG, "deposit: flags must be 0");
    if (!deposit_lattice(c, spec->refine, a, voxels)) return fail(c, PSAMD_ERR_INVALID_ARG, "deposit: refine is not 1, 2 or 4");
    if (!spec->out || !aligned(spec->out, 4) || !aligned(spec->result_dev, 8))
        return fail(c, PSAMD_ERR_INVALID_ARG, "deposit: out missing or misaligned, or result_dev misaligned");
    if (spec->capacity < voxels) return fail(c, PSAMD_ERR_INVALID_ARG, "deposit: capacity is less than (grid_dim * refine)^3");
    PS_TRY(frame_ready(c, "deposit"));
    a.out = spec->out; a.result = spec->result_dev;
    PS_HIP(c, launch_deposit(c->stream, c->P, c->d, a, c->dep));
    return PSAMD_OK;
}

int psamd_deposit_result_get(psamd_ctx *c, psamd_deposit_result *out) { return read_own(c, out, c ? c->dep.own : nullptr, sizeof *out); }

// the same pass into the staging buffer, zeroed first: the voxels this rank does not serve are +0 in the host's array
int psamd_download_deposit(psamd_ctx *c, int32_t refine, float *out, int64_t capacity, psamd_deposit_result *result)
{
    PS_TRY(service_args(c, out));
    DepositArgs a{};
    int64_t voxels = 0;
    if (!deposit_lattice(c, refine, a, voxels)) return fail(c, PSAMD_ERR_INVALID_ARG, "download_deposit: refine is not 1, 2 or 4");
    if (capacity < voxels) return fail(c, PSAMD_ERR_INVALID_ARG, "download_deposit: capacity is less than (grid_dim * refine)^3");
    PS_TRY(frame_ready(c, "download_deposit"));
    const size_t bytes = (size_t)voxels * sizeof(float);
    PS_TRY(ensure_staging(c, std::max<size_t>(bytes, 256)));
    PS_HIP(c, hipMemsetAsync(c->staging, 0, bytes, c->stream));
    a.out = (float *)c->staging; a.result = nullptr;
    PS_HIP(c, launch_deposit(c->stream, c->P, c->d, a, c->dep));
    PS_HIP(c, hipMemcpyAsync(out, c->staging, bytes, hipMemcpyDeviceToHost, c->stream));
    if (result) PS_HIP(c, hipMemcpyAsync(result, c->dep.own, sizeof *result, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    return PSAMD_OK;
}

// ---- a lattice field at the particles (sample.hip) ----
int psamd_sample(psamd_ctx *c, const psamd_sample_spec *spec)
{
    PS_TRY(service_args(c, spec));
    SampleArgs a{};
    int64_t voxels = 0;
    const bool vec4 = (spec->flags & PSAMD_SAMPLE_VEC4) != 0, order = (spec->flags & PSAMD_SAMPLE_EXPORT_ORDER) != 0, some = spec->max_count > 0;
    if ((spec->flags & ~(PSAMD_SAMPLE_VEC4 | PSAMD_SAMPLE_EXPORT_ORDER)) || spec->reserved != 0)
        return fail(c, PSAMD_ERR_INVALID_ARG, "sample: unknown flag bits, or reserved not 0");
    if (!deposit_lattice(c, spec->refine, a, voxels)) return fail(c, PSAMD_ERR_INVALID_ARG, "sample: refine is not 1, 2 or 4");
    if (spec->capacity < voxels) return fail(c, PSAMD_ERR_INVALID_ARG, "sample: capacity is less than (grid_dim * refine)^3");
    if (spec->max_count < 0 || spec->max_count > INT32_MAX) return fail(c, PSAMD_ERR_INVALID_ARG, "sample: max_count outside [0, 2^31)");
    if (!spec->field || (some && !spec->out)) return fail(c, PSAMD_ERR_INVALID_ARG, "sample: field missing, or out missing");
    if (order ? spec->pos4 != nullptr : some && !spec->pos4)
        return fail(c, PSAMD_ERR_INVALID_ARG, "sample: pos4 missing, or given with PSAMD_SAMPLE_EXPORT_ORDER");
    const size_t word = vec4 ? 16 : 4;
    if (!aligned(spec->pos4, 16) || !aligned(spec->field, word) || !aligned(spec->out, word) || !aligned(spec->outcome_dev, 4) ||
        !aligned(spec->count_dev, 8) || !aligned(spec->result_dev, 8))
        return fail(c, PSAMD_ERR_INVALID_ARG, "sample: an array misaligned");
    if (order && !update_window(c->stage))
        return fail(c, PSAMD_ERR_STATE, "sample: between slab_apply and slab_finish the departing particles are staged (by export order "
                                        "their entries would pair with no export)");
    psamd_sample_result *res = spec->result_dev ? spec->result_dev : c->smp.own;
    if (!some) return zero_result(c, c->smp.own, res, sizeof *res);
    a.flags = spec->flags; a.scale = spec->scale; a.field = spec->field; a.pos4 = (const float4 *)spec->pos4;
    a.max_count = spec->max_count; a.count_dev = spec->count_dev; a.out = spec->out; a.outcome = spec->outcome_dev; a.result = res;
    PS_HIP(c, launch_sample(c->stream, c->P, c->d, a, c->smp, c->upd.tile_live));
    return PSAMD_OK;
}

int psamd_sample_result_get(psamd_ctx *c, psamd_sample_result *out) { return read_own(c, out, c ? c->smp.own : nullptr, sizeof *out); }

// ---- neighbours within a radius (neighbours.hip) ----
// the arguments of psamd_neighbours and of its host form (device: the kernels store to the arrays), in the services' order:
// flags, the radius, pointers and alignment, the context kind
static int neighbours_args(psamd_ctx *c, uint32_t flags, float radius, const void *count, const void *nearest, const void *nearest_d2,
                           const void *offsets, int64_t capacity, const void *list, int64_t list_capacity, const void *result, bool device)
{
    if (flags & ~PSAMD_NEIGHBOURS_INDEX) return fail(c, PSAMD_ERR_INVALID_ARG, "neighbours: unknown flag bits");
    if (!std::isfinite(radius) || !(radius > 0.f) || !((double)radius <= c->P.cell_size))
        return fail(c, PSAMD_ERR_INVALID_ARG, "neighbours: radius is not finite, not > 0 or exceeds cell_size (the walk is over the 27-cell stencil)");
    if (capacity < 0 || list_capacity < 0) return fail(c, PSAMD_ERR_INVALID_ARG, "neighbours: capacity < 0 or list_capacity < 0");
    if (device && (!aligned(count, 4) || !aligned(nearest, 4) || !aligned(nearest_d2, 4) || !aligned(list, 4) || !aligned(offsets, 8) ||
                   !aligned(result, 8)))
        return fail(c, PSAMD_ERR_INVALID_ARG, "neighbours: an array misaligned");
    if (list && !offsets) return fail(c, PSAMD_ERR_INVALID_ARG, "neighbours: list needs offsets");
    if ((flags & PSAMD_NEIGHBOURS_INDEX) && c->P.world > 1)
        return fail(c, PSAMD_ERR_UNSUPPORTED, "neighbours: PSAMD_NEIGHBOURS_INDEX is served on one context only (world == 1): a halo's particle "
                                              "has no export index here");
    if ((c->P.flags & PSAMD_FLAG_ALL_PAIRS) && c->P.world > 1)
        return fail(c, PSAMD_ERR_UNSUPPORTED, "neighbours: all-pairs contexts are served on one context only (world == 1)");
    return PSAMD_OK;
}

// the scratch: one block, made by the first call (hipMalloc may wait for the device and cannot be recorded) and kept
static int neighbours_scratch(psamd_ctx *c)
{
    if (c->nbr.block) return PSAMD_OK;
    PS_TRY(refuse_capture(c, "neighbours", "the first call allocates the scratch"));
    void *block = nullptr;
    PS_HIP(c, hipMalloc(&block, neighbours_scratch_bytes(c->P)));
    neighbours_scratch_carve(c->P, block, c->nbr);
    PS_HIP(c, hipMemsetAsync(c->nbr.own, 0, sizeof(NbrOut), c->stream));
    return PSAMD_OK;
}

int psamd_neighbours(psamd_ctx *c, const psamd_neighbours_spec *spec)
{
    PS_TRY(service_args(c, spec));
    PS_TRY(neighbours_args(c, spec->flags, spec->radius, spec->count, spec->nearest, spec->nearest_d2, spec->offsets, spec->capacity,
                           spec->list, spec->list_capacity, spec->result_dev, true));
    PS_TRY(window_nothing_lent(c, "neighbours"));
    PS_TRY(neighbours_scratch(c));
    const NbrArgs a{spec->flags, spec->radius * spec->radius, spec->count, spec->nearest, spec->nearest_d2, spec->offsets, spec->capacity,
                    spec->list, spec->list_capacity, spec->result_dev};
    PS_HIP(c, launch_neighbours(c->stream, c->P, c->d, a, c->nbr));
    return PSAMD_OK;
}

int psamd_neighbours_result_get(psamd_ctx *c, psamd_neighbours_result *out)
{
    PS_TRY(service_args(c, out));
    if (!c->nbr.block) { *out = psamd_neighbours_result{}; out->d2_min = HUGE_VAL; return PSAMD_OK; }     // no call yet
    return read_own(c, out, &c->nbr.own->result, sizeof *out);
}

// the same passes into the staging buffer: what was asked for of the first min(live, capacity) particles, then -- the lists --
// the first min(wanted, list_capacity) names
int psamd_download_neighbours(psamd_ctx *c, uint32_t flags, float radius, int32_t *count, int32_t *nearest, float *nearest_d2, int64_t *offsets,
                              int64_t capacity, int32_t *list, int64_t list_capacity, psamd_neighbours_result *result)
{
    if (!c) return PSAMD_ERR_INVALID_ARG;
    if (c->wedged) return refuse_wedged(c);
    PS_TRY(neighbours_args(c, flags, radius, count, nearest, nearest_d2, offsets, capacity, list, list_capacity, result, false));
    PS_TRY(window_nothing_lent(c, "download_neighbours"));
    PS_TRY(neighbours_scratch(c));
    const int64_t n = std::min<int64_t>(capacity, c->P.slots_total);
    void *const host[5] = {offsets, count, nearest, nearest_d2, list};
    const size_t words[5] = {(size_t)n + 1, (size_t)n, (size_t)n, (size_t)n, (size_t)list_capacity}, width[5] = {8, 4, 4, 4, 4};
    size_t off[5], bytes = 0;
    for (int k = 0; k < 5; k++) { off[k] = bytes; if (host[k]) bytes += (words[k] * width[k] + 255) / 256 * 256; }
    PS_TRY(ensure_staging(c, std::max<size_t>(bytes, 256)));
    void *dev[5];
    for (int k = 0; k < 5; k++) dev[k] = host[k] ? (char *)c->staging + off[k] : nullptr;
    const NbrArgs a{flags, radius * radius, (int *)dev[1], (int *)dev[2], (float *)dev[3], (int64_t *)dev[0], n, (int *)dev[4], list_capacity, nullptr};
    PS_HIP(c, launch_neighbours(c->stream, c->P, c->d, a, c->nbr));
    NbrOut got{};
    PS_HIP(c, hipMemcpyAsync(&got, c->nbr.own, sizeof got, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    const size_t m = (size_t)std::min<int64_t>(got.live, n);
    const size_t take[5] = {m + 1, m, m, m, (size_t)std::min<int64_t>(got.result.wanted, list_capacity)};
    for (int k = 0; k < 5; k++)
        if (host[k] && take[k] > 0) PS_HIP(c, hipMemcpyAsync(host[k], dev[k], take[k] * width[k], hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    if (result) *result = got.result;
    return PSAMD_OK;
}

// ---- groups within a radius (groups.hip) ----
// the arguments of psamd_groups and of its host form, in psamd_neighbours' order; then the context kind: one context only
static int groups_args(psamd_ctx *c, uint32_t flags, float radius, const void *group, int64_t capacity, const void *group_first,
                       const void *group_size, int64_t group_capacity, const void *result, bool device)
{
    if (flags & ~PSAMD_GROUPS_INDEX) return fail(c, PSAMD_ERR_INVALID_ARG, "groups: unknown flag bits");
    if (!std::isfinite(radius) || !(radius > 0.f) || !((double)radius <= c->P.cell_size))
        return fail(c, PSAMD_ERR_INVALID_ARG, "groups: radius is not finite, not > 0 or exceeds cell_size (the walk is over the 27-cell stencil)");
    if (capacity < 0 || group_capacity < 0) return fail(c, PSAMD_ERR_INVALID_ARG, "groups: capacity < 0 or group_capacity < 0");
    if (device && (!aligned(group, 4) || !aligned(group_first, 4) || !aligned(group_size, 4) || !aligned(result, 8)))
        return fail(c, PSAMD_ERR_INVALID_ARG, "groups: an array misaligned");
    if (c->P.world > 1)
        return fail(c, PSAMD_ERR_UNSUPPORTED, "groups: served on one context only (world == 1): a group can span ranks, and the ranks' groups "
                                              "are not merged");
    return PSAMD_OK;
}

// the scratch: one block, made by the first call and kept (neighbours_scratch's rules)
static int groups_scratch(psamd_ctx *c)
{
    if (c->grp.block) return PSAMD_OK;
    PS_TRY(refuse_capture(c, "groups", "the first call allocates the scratch"));
    void *block = nullptr;
    PS_HIP(c, hipMalloc(&block, groups_scratch_bytes(c->P)));
    groups_scratch_carve(c->P, block, c->grp);
    PS_HIP(c, hipMemsetAsync(c->grp.own, 0, sizeof(GrpOut), c->stream));
    return PSAMD_OK;
}

int psamd_groups(psamd_ctx *c, const psamd_groups_spec *spec)
{
    PS_TRY(service_args(c, spec));
    PS_TRY(groups_args(c, spec->flags, spec->radius, spec->group, spec->capacity, spec->group_first, spec->group_size, spec->group_capacity,
                       spec->result_dev, true));
    PS_TRY(frame_ready(c, "groups"));
    PS_TRY(groups_scratch(c));
    const GrpArgs a{spec->flags, spec->radius * spec->radius, spec->group, spec->capacity, spec->group_first, spec->group_size,
                    spec->group_capacity, spec->result_dev};
    PS_HIP(c, launch_groups(c->stream, c->P, c->d, a, c->grp));
    return PSAMD_OK;
}

int psamd_groups_result_get(psamd_ctx *c, psamd_groups_result *out)
{
    PS_TRY(service_args(c, out));
    if (!c->grp.block) { *out = psamd_groups_result{}; return PSAMD_OK; }     // no call yet
    return read_own(c, out, &c->grp.own->result, sizeof *out);
}

// the same passes into the staging buffer: group[] of the first min(live, capacity) particles, the tables' first
// min(groups, group_capacity) entries (there are no more groups than owned slots)
int psamd_download_groups(psamd_ctx *c, uint32_t flags, float radius, int32_t *group, int64_t capacity, int32_t *group_first,
                          int32_t *group_size, int64_t group_capacity, psamd_groups_result *result)
{
    if (!c) return PSAMD_ERR_INVALID_ARG;
    if (c->wedged) return refuse_wedged(c);
    PS_TRY(groups_args(c, flags, radius, group, capacity, group_first, group_size, group_capacity, result, false));
    PS_TRY(frame_ready(c, "download_groups"));
    PS_TRY(groups_scratch(c));
    const int64_t n = std::min<int64_t>(capacity, c->P.slots_total), ng = std::min<int64_t>(group_capacity, c->P.slots_total);
    void *const host[3] = {group, group_first, group_size};
    const size_t words[3] = {(size_t)n, (size_t)ng, (size_t)ng};
    size_t off[3], bytes = 0;
    for (int k = 0; k < 3; k++) { off[k] = bytes; if (host[k]) bytes += (words[k] * 4 + 255) / 256 * 256; }
    PS_TRY(ensure_staging(c, std::max<size_t>(bytes, 256)));
    void *dev[3];
    for (int k = 0; k < 3; k++) dev[k] = host[k] ? (char *)c->staging + off[k] : nullptr;
    const GrpArgs a{flags, radius * radius, (int *)dev[0], n, (int *)dev[1], (int *)dev[2], ng, nullptr};
    PS_HIP(c, launch_groups(c->stream, c->P, c->d, a, c->grp));
    GrpOut got{};
    PS_HIP(c, hipMemcpyAsync(&got, c->grp.own, sizeof got, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    const size_t m = (size_t)std::min<int64_t>(got.live, n), mg = (size_t)std::min<int64_t>(got.result.groups, ng);
    const size_t take[3] = {m, mg, mg};
    for (int k = 0; k < 3; k++)
        if (host[k] && take[k] > 0) PS_HIP(c, hipMemcpyAsync(host[k], dev[k], take[k] * 4, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    if (result) *result = got.result;
    return PSAMD_OK;
}

// ---- the k nearest within a radius (knn.hip) ----
// the arguments of psamd_knn and of its host form, in psamd_neighbours' order; then the context kind
static int knn_args(psamd_ctx *c, uint32_t flags, float radius, int32_t k, int32_t reserved, const void *found, const void *who,
                    const void *d2, int64_t capacity, const void *result, bool device)
{
    if (flags & ~PSAMD_KNN_INDEX) return fail(c, PSAMD_ERR_INVALID_ARG, "knn: unknown flag bits");
    if (reserved != 0) return fail(c, PSAMD_ERR_INVALID_ARG, "knn: reserved must be 0");
    if (!std::isfinite(radius) || !(radius > 0.f) || !((double)radius <= c->P.cell_size))
        return fail(c, PSAMD_ERR_INVALID_ARG, "knn: radius is not finite, not > 0 or exceeds cell_size (the walk is over the 27-cell stencil)");
    if (k < 1 || k > PSAMD_KNN_MAX_K) return fail(c, PSAMD_ERR_INVALID_ARG, "knn: k outside 1 .. PSAMD_KNN_MAX_K");
    if (capacity < 0 || capacity >= ((int64_t)1 << 62) / k) return fail(c, PSAMD_ERR_INVALID_ARG, "knn: capacity < 0, or capacity * k not below 2^62");
    if (device && (!aligned(found, 4) || !aligned(who, 4) || !aligned(d2, 4) || !aligned(result, 8)))
        return fail(c, PSAMD_ERR_INVALID_ARG, "knn: an array misaligned");
    if ((flags & PSAMD_KNN_INDEX) && c->P.world > 1)
        return fail(c, PSAMD_ERR_UNSUPPORTED, "knn: PSAMD_KNN_INDEX is served on one context only (world == 1): a halo's particle has no "
                                              "export index here");
    if ((c->P.flags & PSAMD_FLAG_ALL_PAIRS) && c->P.world > 1)
        return fail(c, PSAMD_ERR_UNSUPPORTED, "knn: all-pairs contexts are served on one context only (world == 1)");
    return PSAMD_OK;
}

// the scratch: one block, made by the first call and kept (neighbours_scratch's rules)
static int knn_scratch(psamd_ctx *c)
{
    if (c->knn.block) return PSAMD_OK;
    PS_TRY(refuse_capture(c, "knn", "the first call allocates the scratch"));
    void *block = nullptr;
    PS_HIP(c, hipMalloc(&block, knn_scratch_bytes(c->P)));
    knn_scratch_carve(c->P, block, c->knn);
    PS_HIP(c, hipMemsetAsync(c->knn.own, 0, sizeof(KnnOut), c->stream));
    return PSAMD_OK;
}

int psamd_knn(psamd_ctx *c, const psamd_knn_spec *spec)
{
    PS_TRY(service_args(c, spec));
    PS_TRY(knn_args(c, spec->flags, spec->radius, spec->k, spec->reserved, spec->found, spec->who, spec->d2, spec->capacity, spec->result_dev, true));
    PS_TRY(window_nothing_lent(c, "knn"));
    PS_TRY(knn_scratch(c));
    const KnnArgs a{spec->flags, spec->radius * spec->radius, spec->k, spec->found, spec->who, spec->d2, spec->capacity, spec->result_dev};
    PS_HIP(c, launch_knn(c->stream, c->P, c->d, a, c->knn));
    return PSAMD_OK;
}

int psamd_knn_result_get(psamd_ctx *c, psamd_knn_result *out)
{
    PS_TRY(service_args(c, out));
    if (!c->knn.block) { *out = psamd_knn_result{}; out->dk2_min = HUGE_VAL; out->dk2_max = -HUGE_VAL; return PSAMD_OK; }     // no call yet
    return read_own(c, out, &c->knn.own->result, sizeof *out);
}

// the same passes into the staging buffer: found and the rows of the first min(live, capacity) particles
int psamd_download_knn(psamd_ctx *c, uint32_t flags, float radius, int32_t k, int32_t *found, int32_t *who, float *d2, int64_t capacity,
                       psamd_knn_result *result)
{
    if (!c) return PSAMD_ERR_INVALID_ARG;
    if (c->wedged) return refuse_wedged(c);
    PS_TRY(knn_args(c, flags, radius, k, 0, found, who, d2, capacity, result, false));
    PS_TRY(window_nothing_lent(c, "download_knn"));
    PS_TRY(knn_scratch(c));
    const int64_t n = std::min<int64_t>(capacity, c->P.slots_total);
    void *const host[3] = {found, who, d2};
    const size_t words[3] = {(size_t)n, (size_t)n * (size_t)k, (size_t)n * (size_t)k};
    size_t off[3], bytes = 0;
    for (int i = 0; i < 3; i++) { off[i] = bytes; if (host[i]) bytes += (words[i] * 4 + 255) / 256 * 256; }
    PS_TRY(ensure_staging(c, std::max<size_t>(bytes, 256)));
    void *dev[3];
    for (int i = 0; i < 3; i++) dev[i] = host[i] ? (char *)c->staging + off[i] : nullptr;
    const KnnArgs a{flags, radius * radius, k, (int *)dev[0], (int *)dev[1], (float *)dev[2], n, nullptr};
    PS_HIP(c, launch_knn(c->stream, c->P, c->d, a, c->knn));
    KnnOut got{};
    PS_HIP(c, hipMemcpyAsync(&got, c->knn.own, sizeof got, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    const size_t m = (size_t)std::min<int64_t>(got.live, n);
    const size_t take[3] = {m, m * (size_t)k, m * (size_t)k};
    for (int i = 0; i < 3; i++)
        if (host[i] && take[i] > 0) PS_HIP(c, hipMemcpyAsync(host[i], dev[i], take[i] * 4, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(c, hipStreamSynchronize(c->stream));
    if (result) *result = got.result;
    return PSAMD_OK;
}

}  // extern "C"
