// update.hip -- psamd_update: new words for particles that stay where they are, on the stream.
//
// An entry names a live particle and carries the words the call's fields ask for: vx, vy, vz (set, or added: a kick),
// age, w, fertility age.  Nothing else of the slot is touched, no queue, no counter: the kernels read the cell array,
// the caller's arrays and -- only for a kick -- vel4, and write the named words (include/psamd.h, "changing particles
// in place").  Only the arrays a call's fields name are read or written; a word that is SET is stored without a load
// (a 16-byte store where x, y, z and w of a float4 are all given, a 12- or 4-byte one otherwise, as ForceBuf::put_slot
// stores acc4.xyz), so SET moves 16 bytes per particle at most and a kick 32 of vel4.
//
// By id, the entries in entry order, three launches ordered by the launch boundaries only, behind a memset of the five
// outcome counters:
//   k_update_claim   per entry: remove_classify (multisplit.hpp: valid id, owned, live), the code kept for the next
//                    launch; atomicMin of the entry's index into the slot's claim word -- remove.hip's claim words, so
//                    the slot's FIRST occurrence wins whatever order the atomics arrive in
//   k_update_write   one lane per entry: the winner (claim == its index) stores its words and restores the claim word
//                    (the claim array is never cleared as a whole: psamd_remove finds it as it left it, and the other way
//                    round); every entry's outcome; the outcomes counted by wave ballot, one atomic per wave and outcome
//   k_update_finish  one thread: the context's own result record and the caller's
// By export order -- the streaming form, every particle every step -- entry k belongs to the k-th live owned slot in
// ascending slot id, psamd_export_live's and phi[]'s pairing, by slot_walk.hpp's walk:
//   k_update_count   one workgroup per tile of SLOT_TILE owned slots: the tile's live count (the cell array alone;
//                    export.hip's count pass also reads pos4 and vel4 for the statistics and is not shared)
//   k_update_order   workgroup 1 + t: a live slot's k from tiles_before, wave_offset and lane_rank; entry k is read and the
//                    slot's words are written, a batch's loads in flight together.  Live slots lie at the heads of their
//                    segments, so the entries read and the slots written by a wave are contiguous runs.  Workgroup 0: the
//                    result record, and outcome 1 for the entries at or past the live count.
//
// VGPRs / waves per SIMD as the compiler reports them for gfx950, no kernel with scratch or LDS beyond slot_walk.hpp's:
//   k_update_claim 6 / 8    k_update_write 18 / 8    k_update_finish 6 / 8    k_update_count 10 / 8    k_update_order 82 / 5
// (k_update_order keeps a batch's entries and old velocities in registers beside the tile's sixteen ballots; it moves
// bytes and computes next to nothing, and five waves per SIMD keep its loads in flight)
#include "multisplit.hpp"

namespace psamd {

// outcome codes (include/psamd.h) and the header words they are counted in
enum { UPD_UPDATED = 0, UPD_NOT_LIVE = ID_NOT_LIVE, UPD_FOREIGN = ID_FOREIGN, UPD_INVALID = ID_INVALID, UPD_DUPLICATE = 4 };
static_assert(UPD_DUPLICATE < UPDATE_HDR_WORDS, "a counter per outcome");
constexpr int UPDATE_BATCH = 4;                                 // slots per lane whose loads are in flight together

// a kick: the slot's vel4 word `o` and the entry's `v` -- one fp32 addition per component, no clamp (the next step's MAX_V
// clamp acts as it always does); the age is the entry's if the fields name it, else the slot's
__device__ __forceinline__ float4 update_kick(uint32_t fields, const float4 o, const float4 v)
{
    return make_float4(__fadd_rn(o.x, v.x), __fadd_rn(o.y, v.y), __fadd_rn(o.z, v.z), (fields & PSAMD_UPDATE_AGE) ? v.w : o.w);
}

// the caller's arrays at entry k into the slot at storage index si: the words the fields name, every other word keeps its
// bits.  o: the slot's vel4 word, loaded by the caller for a kick (PSAMD_UPDATE_ADD) and not looked at otherwise
__device__ __forceinline__ void update_store(uint32_t fields, int si, const float4 o, const float4 v, float w, float fert, float4 *d_pos4,
                                             float4 *d_vel4, float4 *d_acc4)
{
    if (fields & PSAMD_UPDATE_ADD) d_vel4[si] = update_kick(fields, o, v);
    else if ((fields & (PSAMD_UPDATE_VEL | PSAMD_UPDATE_AGE)) == (PSAMD_UPDATE_VEL | PSAMD_UPDATE_AGE)) d_vel4[si] = v;
    else if (fields & PSAMD_UPDATE_VEL) *reinterpret_cast<float3 *>(d_vel4 + si) = make_float3(v.x, v.y, v.z);
    else if (fields & PSAMD_UPDATE_AGE) reinterpret_cast<float *>(d_vel4 + si)[3] = v.w;
    if (fields & PSAMD_UPDATE_MASS) reinterpret_cast<float *>(d_pos4 + si)[3] = w;
    if (fields & PSAMD_UPDATE_FERT) reinterpret_cast<float *>(d_acc4 + si)[3] = fert;
}

__device__ __forceinline__ void update_write_result(long long done, long long updated, long long not_live, long long foreign,
                                                    long long invalid, long long duplicate, psamd_update_result *own,
                                                    psamd_update_result *out)
{
    psamd_update_result res;
    res.done = done; res.updated = updated; res.not_live = not_live; res.foreign = foreign; res.invalid = invalid; res.duplicate = duplicate;
    write_result(own, out, res);
}

// ---- by id ----

__global__ void __launch_bounds__(256) k_update_claim(DevParams P, int64_t max_count, const int64_t *count_dev, const int *__restrict__ ids,
                                                      const int *__restrict__ cell, int *__restrict__ code, int *__restrict__ claim)
{
    const int n = entry_count(count_dev, max_count);
    const int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i64 >= n) return;
    const int si = remove_classify(P, ids[i64], cell);
    code[i64] = si;
    if (si >= 0) atomicMin(&claim[si], (int)i64);
}

__global__ void __launch_bounds__(256) k_update_write(uint32_t fields, int64_t max_count, const int64_t *count_dev,
                                                      const int *__restrict__ code, int *claim, const float4 *__restrict__ vel4,
                                                      const float *__restrict__ w, const float *__restrict__ fert,
                                                      int *__restrict__ outcome, int *__restrict__ hdr, float4 *d_pos4, float4 *d_vel4,
                                                      float4 *d_acc4)
{
    const int n = entry_count(count_dev, max_count);
    const int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int oc = -1;
    if (i64 < n) {
        const int i = (int)i64, si = code[i];
        // The slot's claim word holds its first occurrence's index until that entry's lane restores INT_MAX, in this launch:
        // a later occurrence reads the one or the other, and neither is its own index -- it decides the same thing.
        oc = si < 0 ? -1 - si : claim[si] == i ? UPD_UPDATED : UPD_DUPLICATE;
        if (oc == UPD_UPDATED) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f), o = v;
            if (fields & (PSAMD_UPDATE_VEL | PSAMD_UPDATE_AGE)) v = vel4[i];
            if (fields & PSAMD_UPDATE_ADD) o = d_vel4[si];
            update_store(fields, si, o, v, (fields & PSAMD_UPDATE_MASS) ? w[i] : 0.f, (fields & PSAMD_UPDATE_FERT) ? fert[i] : 0.f, d_pos4,
                         d_vel4, d_acc4);
            claim[si] = INT_MAX;
        }
        if (outcome) outcome[i] = oc;
    }
#pragma unroll
    for (int k = UPD_UPDATED; k <= UPD_DUPLICATE; k++) {
        const int cnt = __popcll(__ballot(oc == k));
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&hdr[k], cnt);
    }
}

__global__ void k_update_finish(int64_t max_count, const int64_t *count_dev, const int *__restrict__ hdr, psamd_update_result *own,
                                psamd_update_result *out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    update_write_result(entry_count(count_dev, max_count), hdr[UPD_UPDATED], hdr[UPD_NOT_LIVE], hdr[UPD_FOREIGN], hdr[UPD_INVALID],
                        hdr[UPD_DUPLICATE], own, out);
}

// ---- by export order ----

__global__ void __launch_bounds__(SLOT_THREADS) k_update_count(DevParams P, const int *__restrict__ cell, int *__restrict__ tile_live)
{
    __shared__ int s_n[SLOT_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x;
    const int first = slot_first(t, wv, lane);
    int live = 0;
#pragma unroll
    for (int k = 0; k < SLOT_ITEMS; k++) live += __popcll(__ballot(slot_live(P, slot_cell(P, cell, first + 64 * k))));
    if (lane == 0) s_n[wv] = live;
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0;
        for (int w = 0; w < SLOT_WAVES; w++) a += s_n[w];
        tile_live[t] = a;
    }
}

__global__ void __launch_bounds__(SLOT_THREADS) k_update_order(DevParams P, uint32_t fields, int ntiles, int64_t max_count,
                                                               const int64_t *count_dev, const int *__restrict__ cell,
                                                               const int *__restrict__ tile_live, const float4 *__restrict__ vel4,
                                                               const float *__restrict__ w, const float *__restrict__ fert,
                                                               int *__restrict__ outcome, psamd_update_result *own,
                                                               psamd_update_result *out, float4 *d_pos4, float4 *d_vel4, float4 *d_acc4)
{
    const int n = entry_count(count_dev, max_count);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (blockIdx.x == 0) {
        // the live count (every tile is "before" tile ntiles, and no wave adds a share of its own)
        const int live = wave_offset<int>(tiles_before(tile_live, ntiles), 0, wv, lane);
        const int updated = min(n, live);
        if (threadIdx.x == 0) update_write_result(n, updated, n - updated, 0, 0, 0, own, out);
        if (outcome) for (int64_t k = (int64_t)live + threadIdx.x; k < n; k += SLOT_THREADS) outcome[k] = UPD_NOT_LIVE;
        return;
    }
    const int t = blockIdx.x - 1;
    const int before = tiles_before(tile_live, t);        // the live particles of the tiles before this one
    const int first = slot_first(t, wv, lane);
    unsigned long long mask[SLOT_ITEMS];
    int live = 0;
#pragma unroll
    for (int k = 0; k < SLOT_ITEMS; k++) {
        mask[k] = __ballot(slot_live(P, slot_cell(P, cell, first + 64 * k)));
        live += __popcll(mask[k]);
    }
    int at = wave_offset<int>(before, live, wv, lane);
    if (at >= n) return;                                  // (the wave's live slots all fall past the entries: left alone)
    const bool add = (fields & PSAMD_UPDATE_ADD) != 0, vel = (fields & (PSAMD_UPDATE_VEL | PSAMD_UPDATE_AGE)) != 0;
    // a batch's loads together, then its stores
#pragma unroll
    for (int k0 = 0; k0 < SLOT_ITEMS; k0 += UPDATE_BATCH) {
        float4 v[UPDATE_BATCH], o[UPDATE_BATCH];
        float nw[UPDATE_BATCH], nf[UPDATE_BATCH];
        int e[UPDATE_BATCH];
#pragma unroll
        for (int k = 0; k < UPDATE_BATCH; k++) {
            const unsigned long long m = mask[k0 + k];
            e[k] = ((m >> lane) & 1ull) ? at + lane_rank(m) : INT_MAX;
            at += __popcll(m);
            v[k] = o[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            nw[k] = nf[k] = 0.f;
            if (e[k] < n) {
                if (vel) v[k] = vel4[e[k]];
                if (add) o[k] = d_vel4[first + 64 * (k0 + k)];
                if (fields & PSAMD_UPDATE_MASS) nw[k] = w[e[k]];
                if (fields & PSAMD_UPDATE_FERT) nf[k] = fert[e[k]];
            }
        }
#pragma unroll
        for (int k = 0; k < UPDATE_BATCH; k++) {
            if (e[k] >= n) continue;
            update_store(fields, first + 64 * (k0 + k), o[k], v[k], nw[k], nf[k], d_pos4, d_vel4, d_acc4);
            if (outcome) outcome[e[k]] = UPD_UPDATED;
        }
    }
}

hipError_t launch_update_ids(hipStream_t st, const DevParams &P, const DeviceState &d, const UpdateArgs &a, const UpdateScratch &s,
                             int *claim)
{
    {   const hipError_t e = hipMemsetAsync(s.hdr, 0, UPDATE_HDR_WORDS * sizeof(int), st); if (e != hipSuccess) return e; }
    const unsigned blocks = (unsigned)((a.max_count + 255) / 256);
    k_update_claim<<<blocks, 256, 0, st>>>(P, a.max_count, a.count_dev, a.ids, d.cell, s.code, claim);
    PS_LAUNCH_CHECK();
    k_update_write<<<blocks, 256, 0, st>>>(a.fields, a.max_count, a.count_dev, s.code, claim, a.vel4, a.w, a.fert_age, a.outcome, s.hdr,
                                           d.pos4, d.vel4, d.acc4);
    PS_LAUNCH_CHECK();
    k_update_finish<<<1, 64, 0, st>>>(a.max_count, a.count_dev, s.hdr, s.own, a.result);
    PS_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_live_tiles(hipStream_t st, const DevParams &P, const DeviceState &d, int *tile_live)
{
    const int ntiles = slot_tiles(P.slots_total);
    if (ntiles > 0) {
        k_update_count<<<ntiles, SLOT_THREADS, 0, st>>>(P, d.cell, tile_live);
        PS_LAUNCH_CHECK();
    }
    return hipSuccess;
}

hipError_t launch_update_order(hipStream_t st, const DevParams &P, const DeviceState &d, const UpdateArgs &a, const UpdateScratch &s)
{
    const int ntiles = slot_tiles(P.slots_total);
    {   const hipError_t e = launch_live_tiles(st, P, d, s.tile_live); if (e != hipSuccess) return e; }
    k_update_order<<<ntiles + 1, SLOT_THREADS, 0, st>>>(P, a.fields, ntiles, a.max_count, a.count_dev, d.cell, s.tile_live, a.vel4, a.w,
                                                        a.fert_age, a.outcome, s.own, a.result, d.pos4, d.vel4, d.acc4);
    PS_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace psamd
