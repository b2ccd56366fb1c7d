// remove.hip -- psamd_remove: particles out of their slots and the slots back into their segments' queues, on the stream.
//
// The device-side counterpart of the reference's kill (reset_particle + q_insert of the slot id into the queue of the
// slot's own segment, ps.cpp:1210-1242), byte for byte, for a set of candidates in a defined serial order.  A candidate
// whose slot is live at its turn is reset; the k-th such candidate of a queue record, in that order, is the record's k-th
// q_insert.  No remove interleaves, so the inserts have a closed form in the record's (front, rear, count) before the
// call: the first seg_size - count of them are taken, at the offsets (first + k) % seg_size behind rloc, where
// first = 0 for an empty record (q_insert restarts it at rloc whatever front and rear held) and rear - rloc + 1 otherwise;
// the rest are dropped (a full queue takes nothing; the particle is reset all the same).
//
// By id, the candidates are the caller's entries in entry order, in four launches ordered by the launch boundaries only
// (no hand-off between workgroups):
//   k_remove_claim   per entry whose id is valid, owned and live: atomicMin of the entry's index into the slot's claim
//                    word -- the slot's FIRST occurrence wins, whatever the order the atomics arrive in
//   k_remove_rank    one workgroup per tile of ENTRY_TILE entries: the outcome of the entries that remove nothing, the
//                    record of the winners, their stable rank inside the tile and the tile's per-record counts
//                    (multisplit.hpp, shared with inject.hip)
//   k_remove_commit  one workgroup: per record the exclusive prefix of the tile counts; from the record's total its
//                    insert rule (first offset, room) for the next launch, the record as q_insert leaves it, the result
//   k_remove_place   per winner: the slot reset as k_unpack_aos writes a free slot, its claim word restored (the claim
//                    array is never cleared as a whole), its id at the closed-form position of the queue, the outcome
// By box, the candidates are the selected live particles in ascending slot id.  A record covers one contiguous slot range,
// so a candidate's rank in its record is a prefix count in slot order (slot_walk.hpp):
//   k_remove_box_count   one workgroup per tile of SLOT_TILE owned slots: the tile's selected and live counts
//   k_remove_box_prefix  per slot the number of selected slots before it (the tiles' prefix rebuilt in the workgroup)
//   k_remove_box_commit  one workgroup: per owned record its total from the prefix at its bounds, then as k_remove_commit
//   k_remove_box_place   per selected slot: rank = prefix[slot] - prefix[record's first slot], then as k_remove_place
// The kernels touch the caller's arrays, the scratch, the queues and the slots they free: nothing a step in flight owns
// (stream order puts them between steps).  T_DATA mirror rows are left alone, as the reference's reset leaves them.
#include "multisplit.hpp"

namespace psamd {

// outcome codes (include/psamd.h); an entry that removes nothing is kept as -1 - code in its record word
// (remove_classify, multisplit.hpp, answers with the codes 1, 2, 3)
enum { REM_REMOVED = 0, REM_NOT_LIVE = ID_NOT_LIVE, REM_FOREIGN = ID_FOREIGN, REM_INVALID = ID_INVALID, REM_DROPPED = 4 };

// a free slot as k_unpack_aos writes it (psamd_snapshot_restore relies on free slots being all-zero)
__device__ __forceinline__ void remove_reset(int si, float4 *d_pos4, float4 *d_vel4, float4 *d_acc4, int *d_cell, uint8_t *d_pflags)
{
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    d_pos4[si] = z; d_vel4[si] = z; d_acc4[si] = z;
    d_cell[si] = -1;
    d_pflags[si] = 0;
}

// Record r after R removals, as R serial q_insert leave it; ins = (offset behind rloc of the first insert, inserts the
// queue takes) for the placement.  Returns how many of the R the full queue did not take.
__device__ __forceinline__ int remove_commit_record(QueueInfo *qinfo, int2 *__restrict__ ins, int r, int R)
{
    QueueInfo q = qinfo[r];
    const int room = q.seg_size - q.count, A = min(R, room);
    const int first = q.count == 0 ? 0 : (q.rear - q.rloc + 1) % q.seg_size;
    ins[r] = make_int2(first, room);
    if (A > 0) {
        if (q.count == 0) q.front = q.rloc;
        q.rear = q.rloc + (first + A - 1) % q.seg_size;
        q.count += A;
        qinfo[r] = q;
    }
    return R - A;
}

// the k-th removal of a record: the slot id into the queue (stored like the slots) if the queue takes it
__device__ __forceinline__ int remove_insert(const DevParams &P, const QueueInfo *__restrict__ qinfo, const int2 *__restrict__ ins,
                                             int *__restrict__ queue, int r, int k, int id)
{
    const int2 rule = ins[r];
    if (k >= rule.y) return REM_DROPPED;
    const QueueInfo q = qinfo[r];                       // (rloc and seg_size: the commit does not change them)
    queue[slot_index(P, q.rloc) + (rule.x + k) % q.seg_size] = id;
    return REM_REMOVED;
}

// ---- by id ----

__global__ void k_remove_claim(DevParams P, int64_t max_count, const int64_t *count_dev, const int *__restrict__ ids,
                               const int *__restrict__ cell, int *__restrict__ claim)
{
    const int n = entry_count(count_dev, max_count);
    const int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i64 >= n) return;
    const int si = remove_classify(P, ids[i64], cell);
    if (si >= 0) atomicMin(&claim[si], (int)i64);
}

template <bool LDS>
__global__ void __launch_bounds__(SPLIT_THREADS) k_remove_rank(DevParams P, SegLayout S, int nrec, int64_t max_count, const int64_t *count_dev,
                                                               const int *__restrict__ ids, const int *__restrict__ cell,
                                                               const int *__restrict__ claim, int2 *__restrict__ ent,
                                                               int *__restrict__ tcount, int *__restrict__ tile_out)
{
    extern __shared__ int lds_cnt[];
    __shared__ int s_out[3];
    const int n = entry_count(count_dev, max_count);
    const int t = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (t * ENTRY_TILE >= n) return;
    if (tid < 3) s_out[tid] = 0;
    SplitKeys k;
    split_tile_begin<LDS>(t, nrec, lds_cnt, tcount, k);
#pragma unroll
    for (int g = 0; g < SPLIT_GROUPS; g++) {
        const int i = split_entry(t, g), lane = tid & 63;
        int r = INT_MIN;                                           // past the last entry
        if (i < n) {
            const int id = ids[i];
            const int si = remove_classify(P, id, cell);
            // a later occurrence of a slot finds it gone at its turn: not live
            r = si < 0 ? si : claim[si] == i ? segment_record_of_slot(S, id) : -1 - REM_NOT_LIVE;
        }
        k.rec[g] = r;
        split_group_rank(r, lane, k.in_rank[g], k.pop[g], k.lead[g]);
#pragma unroll
        for (int code = REM_NOT_LIVE; code <= REM_INVALID; code++) {
            const unsigned long long m = __ballot(r == -1 - code);
            if (lane == 0 && m) atomicAdd(&s_out[code - 1], __popcll(m));
        }
    }
    split_tile_store<LDS>(t, n, nrec, k, ent, tcount);
    if (tid < 3) tile_out[3 * t + tid] = s_out[tid];
}

__device__ __forceinline__ void remove_write_result(const long long (&v)[6], psamd_remove_result *own, psamd_remove_result *out)
{
    psamd_remove_result res;
    res.done = v[0]; res.removed = v[1]; res.not_live = v[2]; res.foreign = v[3]; res.invalid = v[4]; res.dropped = v[5];
    write_result(own, out, res);
}

__global__ void __launch_bounds__(1024) k_remove_commit(int nrec, int64_t max_count, const int64_t *count_dev, int *__restrict__ tcount,
                                                        const int *__restrict__ tile_out, QueueInfo *qinfo, int2 *__restrict__ ins,
                                                        psamd_remove_result *own, psamd_remove_result *out)
{
    __shared__ unsigned long long s_sum[6];
    const int n = entry_count(count_dev, max_count), tiles = entry_tiles(n);
    const int tid = (int)threadIdx.x;
    long long v[6] = {0, 0, 0, 0, 0, 0}, sum[6];
    for (int r = tid; r < nrec; r += 1024) {
        const int R = split_tile_prefix(tcount, nrec, tiles, r);
        if (R <= 0) continue;
        v[1] += R;
        v[5] += remove_commit_record(qinfo, ins, r, R);
    }
    for (int t = tid; t < tiles; t += 1024) { v[2] += tile_out[3 * t]; v[3] += tile_out[3 * t + 1]; v[4] += tile_out[3 * t + 2]; }
    block_sum(v, s_sum, sum);
    sum[0] = n;
    if (tid == 0) remove_write_result(sum, own, out);
}

__global__ void k_remove_place(DevParams P, int nrec, int64_t max_count, const int64_t *count_dev, const int *__restrict__ ids,
                               const int2 *__restrict__ ent, const int *__restrict__ tcount, const QueueInfo *__restrict__ qinfo,
                               const int2 *__restrict__ ins, int *__restrict__ queue, int *__restrict__ claim,
                               int *__restrict__ outcome, float4 *d_pos4, float4 *d_vel4, float4 *d_acc4, int *d_cell, uint8_t *d_pflags)
{
    const int n = entry_count(count_dev, max_count);
    const int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i64 >= n) return;
    const int i = (int)i64;
    const int2 e = ent[i];
    int code = -1 - e.x;
    if (e.x >= 0) {
        const int id = ids[i], si = slot_index(P, id);
        const int k = e.y + tcount[(size_t)(i / ENTRY_TILE) * nrec + e.x];
        remove_reset(si, d_pos4, d_vel4, d_acc4, d_cell, d_pflags);
        claim[si] = INT_MAX;
        code = remove_insert(P, qinfo, ins, queue, e.x, k, id);
    }
    if (outcome) outcome[i] = code;
}

// ---- by box ----

struct RemoveBox {
    float lo[3], hi[3];
    int outside;
    // fp32 comparisons: a coordinate that is not a number is not inside
    __device__ __forceinline__ bool selects(const float4 p) const
    {
        const bool in = lo[0] <= p.x && p.x < hi[0] && lo[1] <= p.y && p.y < hi[1] && lo[2] <= p.z && p.z < hi[2];
        return outside ? !in : in;
    }
};

// slot i (storage order) is live, and selected
__device__ __forceinline__ bool remove_box_selected(const DevParams &P, const RemoveBox &B, int i, const int *cell, const float4 *pos4,
                                                    bool &live)
{
    live = i < P.slots_total && slot_live(P, cell[i]);
    return live && B.selects(pos4[i]);
}

__global__ void __launch_bounds__(SLOT_THREADS) k_remove_box_count(DevParams P, RemoveBox B, const int *__restrict__ cell,
                                                                         const float4 *__restrict__ pos4, int *__restrict__ tile_sel,
                                                                         int *__restrict__ tile_live)
{
    __shared__ int s_n[SLOT_WAVES][2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x;
    const int first = slot_first(t, wv, lane);
    int sel = 0, live = 0;
#pragma unroll 4
    for (int k = 0; k < SLOT_ITEMS; k++) {
        bool l;
        const bool s = remove_box_selected(P, B, first + 64 * k, cell, pos4, l);
        sel += __popcll(__ballot(s));
        live += __popcll(__ballot(l));
    }
    if (lane == 0) { s_n[wv][0] = sel; s_n[wv][1] = live; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0, b = 0;
        for (int w = 0; w < SLOT_WAVES; w++) { a += s_n[w][0]; b += s_n[w][1]; }
        tile_sel[t] = a; tile_live[t] = b;
    }
}

// prefix[i]: selected slots before storage index i; prefix[slots_total]: all of them
__global__ void __launch_bounds__(SLOT_THREADS) k_remove_box_prefix(DevParams P, RemoveBox B, int ntiles, const int *__restrict__ cell,
                                                                          const float4 *__restrict__ pos4,
                                                                          const int *__restrict__ tile_sel, int *__restrict__ prefix)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x;
    const int before = tiles_before(tile_sel, t);
    const int first = slot_first(t, wv, lane);
    unsigned long long mask[SLOT_ITEMS];
    int sel = 0;
#pragma unroll
    for (int k = 0; k < SLOT_ITEMS; k++) {
        bool l;
        mask[k] = __ballot(remove_box_selected(P, B, first + 64 * k, cell, pos4, l));
        sel += __popcll(mask[k]);
    }
    int at = wave_offset<int>(before, sel, wv, lane);
#pragma unroll
    for (int k = 0; k < SLOT_ITEMS; k++) {
        const unsigned long long m = mask[k];
        const int i = first + 64 * k;
        if (i < P.slots_total) prefix[i] = at + lane_rank(m);
        at += __popcll(m);
    }
    // (the tile's last wave and lane have walked the whole tile)
    if (t == ntiles - 1 && threadIdx.x == SLOT_THREADS - 1) prefix[P.slots_total] = at;
}

__global__ void __launch_bounds__(1024) k_remove_box_commit(DevParams P, int nrec, int ntiles, const int *__restrict__ prefix,
                                                            const int *__restrict__ tile_live, QueueInfo *qinfo, int2 *__restrict__ ins,
                                                            psamd_remove_result *own, psamd_remove_result *out)
{
    __shared__ unsigned long long s_sum[6];
    const int tid = (int)threadIdx.x;
    long long v[6] = {0, 0, 0, 0, 0, 0}, sum[6];
    for (int r = tid; r < nrec; r += 1024) {
        if (!owns_record(P, r)) continue;
        const int rloc = qinfo[r].rloc, seg = qinfo[r].seg_size, rs = slot_index(P, rloc);
        const int R = prefix[rs + seg] - prefix[rs];
        if (R <= 0) continue;
        v[1] += R;
        v[5] += remove_commit_record(qinfo, ins, r, R);
    }
    for (int t = tid; t < ntiles; t += 1024) v[0] += tile_live[t];
    block_sum(v, s_sum, sum);
    if (tid == 0) remove_write_result(sum, own, out);
}

__global__ void __launch_bounds__(SLOT_THREADS) k_remove_box_place(DevParams P, SegLayout S, RemoveBox B, const int *__restrict__ prefix,
                                                                         const QueueInfo *__restrict__ qinfo, const int2 *__restrict__ ins,
                                                                         int *__restrict__ queue, float4 *d_pos4, float4 *d_vel4,
                                                                         float4 *d_acc4, int *d_cell, uint8_t *d_pflags)
{
    const int i = (int)(blockIdx.x * SLOT_THREADS + threadIdx.x);
    bool live;
    if (!remove_box_selected(P, B, i, d_cell, d_pos4, live)) return;
    const int id = slot_of_index(P, i), r = segment_record_of_slot(S, id);
    const int k = prefix[i] - prefix[slot_index(P, qinfo[r].rloc)];
    remove_reset(i, d_pos4, d_vel4, d_acc4, d_cell, d_pflags);
    (void)remove_insert(P, qinfo, ins, queue, r, k, id);
}

hipError_t launch_remove_ids(hipStream_t st, const DevParams &P, const SegLayout &S, const DeviceState &d, int nrec, const RemoveArgs &a,
                             const RemoveScratch &s)
{
    const int64_t tiles = (a.max_count + ENTRY_TILE - 1) / ENTRY_TILE;
    const unsigned blocks = (unsigned)((a.max_count + 255) / 256);
    k_remove_claim<<<blocks, 256, 0, st>>>(P, a.max_count, a.count_dev, a.ids, d.cell, s.claim);
    PS_LAUNCH_CHECK();
    if (nrec <= SPLIT_LDS_RECORDS)
        k_remove_rank<true><<<(unsigned)tiles, SPLIT_THREADS, (size_t)nrec * sizeof(int), st>>>(P, S, nrec, a.max_count, a.count_dev, a.ids, d.cell,
                                                                                              s.claim, s.e.ent, s.e.tcount, s.e.tile_out);
    else
        k_remove_rank<false><<<(unsigned)tiles, SPLIT_THREADS, 0, st>>>(P, S, nrec, a.max_count, a.count_dev, a.ids, d.cell, s.claim, s.e.ent,
                                                                      s.e.tcount, s.e.tile_out);
    PS_LAUNCH_CHECK();
    k_remove_commit<<<1, 1024, 0, st>>>(nrec, a.max_count, a.count_dev, s.e.tcount, s.e.tile_out, d.qinfo, s.ins, s.own, a.result);
    PS_LAUNCH_CHECK();
    k_remove_place<<<blocks, 256, 0, st>>>(P, nrec, a.max_count, a.count_dev, a.ids, s.e.ent, s.e.tcount, d.qinfo, s.ins, d.queue, s.claim,
                                           a.outcome, d.pos4, d.vel4, d.acc4, d.cell, d.pflags);
    PS_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_remove_box(hipStream_t st, const DevParams &P, const SegLayout &S, const DeviceState &d, int nrec, const float lo[3],
                             const float hi[3], bool outside, psamd_remove_result *result, const RemoveScratch &s)
{
    const int ntiles = slot_tiles(P.slots_total);
    RemoveBox B;
    for (int k = 0; k < 3; k++) { B.lo[k] = lo[k]; B.hi[k] = hi[k]; }
    B.outside = outside ? 1 : 0;
    if (ntiles > 0) {
        k_remove_box_count<<<ntiles, SLOT_THREADS, 0, st>>>(P, B, d.cell, d.pos4, s.tile_sel, s.tile_live);
        PS_LAUNCH_CHECK();
        k_remove_box_prefix<<<ntiles, SLOT_THREADS, 0, st>>>(P, B, ntiles, d.cell, d.pos4, s.tile_sel, s.prefix);
        PS_LAUNCH_CHECK();
    }
    k_remove_box_commit<<<1, 1024, 0, st>>>(P, ntiles > 0 ? nrec : 0, ntiles, s.prefix, s.tile_live, d.qinfo, s.ins, s.own, result);
    PS_LAUNCH_CHECK();
    if (ntiles > 0) {
        k_remove_box_place<<<ntiles * SLOT_ITEMS, SLOT_THREADS, 0, st>>>(P, S, B, s.prefix, d.qinfo, s.ins, d.queue,
                                                                                                      d.pos4, d.vel4, d.acc4, d.cell, d.pflags);
        PS_LAUNCH_CHECK();
    }
    return hipSuccess;
}

}  // namespace psamd
