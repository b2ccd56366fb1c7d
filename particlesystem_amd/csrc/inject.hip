// inject.hip -- psamd_inject: particles from device arrays into their segments' free slots, on the stream.
//
// The device-side counterpart of psamd_fill_particles (io.hip), byte for byte: entry i takes the next free slot of
// its segment's queue in entry order (q_remove), and the stop rule is fill's.  A deterministic stable multisplit of the
// entries by queue record, then the closed-form FIFO removal (the k-th remove of a record takes logical element k, as
// k_replay_commit does), in five launches ordered by the launch boundaries only (no hand-off between workgroups):
//   k_inject_locate  one workgroup per tile of ENTRY_TILE entries: Geometry::locate in fp64, the segment record, the
//                    ownership rule; the tile's per-record counts and every entry's stable rank inside the tile
//                    (multisplit.hpp, shared with remove.hip); the tile's first entry outside the box
//   k_inject_scan    one workgroup: per record, the exclusive prefix of the tile counts (in place) and the first
//                    outside entry of all tiles
//   k_inject_fail    per entry: its rank k among the earlier entries of its record; k == the queue's count is the
//                    record's first queue failure (atomicMin: order-independent)
//   k_inject_place   per entry below F = min(first outside, first failure, n): slot = queue[front + k], the slot written
//                    as k_place writes it, the queue word -1, the id; per record how many it removed
//   k_inject_commit  one workgroup: front / count / rear as host_q_remove leaves them, and the result record
// The kernels touch the entries, the scratch, the queues and the slots they hand out: nothing a step in flight owns
// (stream order puts them between steps).
#include "multisplit.hpp"

namespace psamd {

constexpr int INJ_NOT_MINE = -1, INJ_OUTSIDE = -2;

template <bool LDS>
__global__ void __launch_bounds__(SPLIT_THREADS) k_inject_locate(DevParams P, SegLayout S, int nrec, const CellInfo *__restrict__ celltab,
                                                                 const float4 *__restrict__ pos4, int64_t max_count, const int64_t *count_dev,
                                                                 int2 *__restrict__ ent, int *__restrict__ tcount, int *__restrict__ tile_out)
{
    extern __shared__ int lds_cnt[];
    __shared__ int s_first_out;
    const int n = entry_count(count_dev, max_count);
    const int t = (int)blockIdx.x;
    if (t * ENTRY_TILE >= n) return;
    if (threadIdx.x == 0) s_first_out = INT_MAX;
    SplitKeys k;
    split_tile_begin<LDS>(t, nrec, lds_cnt, tcount, k);
    int first_out = INT_MAX;
#pragma unroll
    for (int g = 0; g < SPLIT_GROUPS; g++) {
        const int i = split_entry(t, g);
        int r = INJ_NOT_MINE;
        if (i < n) {
            const float4 p = pos4[i];
            int cell;
            if (!locate_cell(P, p.x, p.y, p.z, cell)) { r = INJ_OUTSIDE; first_out = min(first_out, i); }
            else {
                const CellInfo ci = celltab[cell];
                const int sr = segment_record(S, ci.seg_type, ci.seg_tid);
                r = owns_record(P, sr) ? sr : INJ_NOT_MINE;
            }
        }
        k.rec[g] = r;
        split_group_rank(r, (int)threadIdx.x & 63, k.in_rank[g], k.pop[g], k.lead[g]);
    }
    if (first_out != INT_MAX) atomicMin(&s_first_out, first_out);
    split_tile_store<LDS>(t, n, nrec, k, ent, tcount);
    if (threadIdx.x == 0) tile_out[t] = s_first_out;
}

// one workgroup: per record the exclusive prefix of the tiles' counts, in tile order, in place; the first entry outside
// the box; the first queue failure's word made ready for k_inject_fail; the removal counts zeroed
__global__ void __launch_bounds__(1024) k_inject_scan(int nrec, int64_t max_count, const int64_t *count_dev, int *__restrict__ tcount,
                                                      const int *__restrict__ tile_out, int *__restrict__ removed, int *__restrict__ hdr)
{
    __shared__ int s_min;
    const int n = entry_count(count_dev, max_count), tiles = entry_tiles(n);
    const int tid = (int)threadIdx.x;
    if (tid == 0) s_min = INT_MAX;
    __syncthreads();
    int m = INT_MAX;
    for (int t = tid; t < tiles; t += 1024) m = min(m, tile_out[t]);
    if (m != INT_MAX) atomicMin(&s_min, m);
    for (int r = tid; r < nrec; r += 1024) {
        (void)split_tile_prefix(tcount, nrec, tiles, r);
        removed[r] = 0;
    }
    __syncthreads();
    if (tid == 0) { hdr[0] = s_min; hdr[1] = INT_MAX; }
}

__global__ void k_inject_fail(int nrec, int64_t max_count, const int64_t *count_dev, const int *__restrict__ tcount,
                              const QueueInfo *__restrict__ qinfo, int2 *__restrict__ ent, int *__restrict__ hdr)
{
    const int n = entry_count(count_dev, max_count);
    const int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i64 >= n) return;
    const int i = (int)i64;
    int2 e = ent[i];
    if (e.x < 0) return;
    e.y += tcount[(size_t)(i / ENTRY_TILE) * nrec + e.x];
    ent[i] = e;
    if (e.y == qinfo[e.x].count) atomicMin(&hdr[1], i);
}

__global__ void k_inject_place(DevParams P, int64_t max_count, const int64_t *count_dev, const float4 *__restrict__ pos4,
                               const float4 *__restrict__ vel4, const float *__restrict__ fert, const int2 *__restrict__ ent,
                               const int *__restrict__ hdr, const QueueInfo *__restrict__ qinfo, int *__restrict__ queue,
                               int *__restrict__ ids, int *__restrict__ removed, float4 *d_pos4, float4 *d_vel4, float4 *d_acc4,
                               int *d_cell, uint8_t *d_pflags)
{
    const int n = entry_count(count_dev, max_count);
    const int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i64 >= n) return;
    const int i = (int)i64;
    const int F = min(min(hdr[0], hdr[1]), n);
    const int2 e = ent[i];
    int slot = -1;
    if (i < F && e.x >= 0) {
        const QueueInfo q = qinfo[e.x];
        const int k = e.y;                                          // < q.count: the first failure is at or after F
        const int off = (q.front - q.rloc + k) % q.seg_size;        // logical element k
        const int qi = slot_index(P, q.rloc) + off;                 // the queue is stored like the slots
        slot = queue[qi];
        queue[qi] = -1;
        const int si = slot_index(P, slot);
        if (si >= 0) {
            const float4 p = pos4[i];
            int cell = -1;
            (void)locate_cell(P, p.x, p.y, p.z, cell);
            d_pos4[si] = p;                                         // create_particle_s, as k_place writes it
            d_vel4[si] = vel4 ? vel4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            d_acc4[si] = make_float4(0.f, 0.f, 0.f, fert ? fert[i] : 0.f);
            d_cell[si] = cell;
            d_pflags[si] = 0;
        }
        atomicMax(&removed[e.x], k + 1);
    }
    if (ids) ids[i] = slot;
}

// one workgroup: every record the entries took slots from, as host_q_remove leaves it after that many removals; the
// result record (the context's own, and the caller's)
__global__ void __launch_bounds__(1024) k_inject_commit(int nrec, int64_t max_count, const int64_t *count_dev, const int *__restrict__ hdr,
                                                        const int *__restrict__ removed, QueueInfo *qinfo, psamd_inject_result *own,
                                                        psamd_inject_result *out)
{
    __shared__ unsigned long long s_placed[1];
    const int n = entry_count(count_dev, max_count);
    const int tid = (int)threadIdx.x;
    long long placed[1] = {0}, sum[1];
    for (int r = tid; r < nrec; r += 1024) {
        const int R = removed[r];
        if (R <= 0) continue;
        QueueInfo q = qinfo[r];
        q.count -= R;
        if (q.count == 0) { q.front = -1; q.rear = -1; }
        else q.front = q.rloc + (q.front - q.rloc + R) % q.seg_size;
        qinfo[r] = q;
        placed[0] += R;
    }
    block_sum(placed, s_placed, sum);
    if (tid == 0) {
        const int fo = hdr[0], ff = hdr[1];
        const int F = min(min(fo, ff), n);
        psamd_inject_result res;
        res.done = F;
        res.placed = sum[0];
        res.status = F == n ? PSAMD_OK : F == fo ? PSAMD_ERR_OUTSIDE_BOX : PSAMD_ERR_QUEUE_EMPTY;
        res.reserved = 0;
        write_result(own, out, res);
    }
}

hipError_t launch_inject(hipStream_t st, const DevParams &P, const SegLayout &S, const DeviceState &d, int nrec, const InjectArgs &a,
                         const InjectScratch &s)
{
    const int64_t tiles = (a.max_count + ENTRY_TILE - 1) / ENTRY_TILE;
    if (nrec <= SPLIT_LDS_RECORDS)
        k_inject_locate<true><<<(unsigned)tiles, SPLIT_THREADS, (size_t)nrec * sizeof(int), st>>>(P, S, nrec, d.celltab, a.pos4, a.max_count,
                                                                                                a.count_dev, s.e.ent, s.e.tcount, s.e.tile_out);
    else
        k_inject_locate<false><<<(unsigned)tiles, SPLIT_THREADS, 0, st>>>(P, S, nrec, d.celltab, a.pos4, a.max_count, a.count_dev,
                                                                        s.e.ent, s.e.tcount, s.e.tile_out);
    PS_LAUNCH_CHECK();
    k_inject_scan<<<1, 1024, 0, st>>>(nrec, a.max_count, a.count_dev, s.e.tcount, s.e.tile_out, s.removed, s.hdr);
    PS_LAUNCH_CHECK();
    const unsigned blocks = (unsigned)((a.max_count + 255) / 256);
    k_inject_fail<<<blocks, 256, 0, st>>>(nrec, a.max_count, a.count_dev, s.e.tcount, d.qinfo, s.e.ent, s.hdr);
    PS_LAUNCH_CHECK();
    k_inject_place<<<blocks, 256, 0, st>>>(P, a.max_count, a.count_dev, a.pos4, a.vel4, a.fert_age, s.e.ent, s.hdr, d.qinfo, d.queue,
                                           a.ids, s.removed, d.pos4, d.vel4, d.acc4, d.cell, d.pflags);
    PS_LAUNCH_CHECK();
    k_inject_commit<<<1, 1024, 0, st>>>(nrec, a.max_count, a.count_dev, s.hdr, s.removed, d.qinfo, s.own, a.result);
    PS_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace psamd
