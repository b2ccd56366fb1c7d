// neighbours.hip -- psamd_neighbours: every listed particle's neighbours within a radius, in CSR form, on the device.
//
// Not part of the step and not in the reference.  The pass reads the frame psamd_build_grid left (cell_start, sorted_id, the
// snap_soa planes, snap_age) and walks, for every particle of the own cells' lists, exactly the bodies the force pass walks for
// its cell (include/psamd.h, "neighbours within a radius", holds the definition), in launches that nothing in between has to
// wait for:
//   k_nbr_count    one wave per (own cell, 64-particle slice), one lane per query (nbr_walk.hpp): the count, and the nearest
//                  pair by (d2, global slot id), by sorted index.
//   k_nbr_reduce   per tile of SLOT_TILE sorted entries: the three words scattered to slot order through sorted_id; the tile's
//                  queries, pairs, largest count and smallest d2; and -- tile t of the owned SLOTS -- its live count.
//   k_nbr_index    per tile of slots: the slot -> export index table, and the sum of the counts of the tile's entries below
//                  the capacity.
//   k_nbr_finish   workgroup 0: the tiles in index order, the result record, offsets[m]; workgroup 1 + t: slot tile t to
//                  export order -- count, nearest, nearest_d2, and offsets as an int64 exclusive scan (the tiles' sums before
//                  t, then inside the tile) -- and every slot's start in the lists.
//   k_nbr_fill     (a list was asked for) k_nbr_count's walk again: each lane stores the names of its neighbours from its
//                  slot's start on, as far as the list's capacity goes.
// The launch boundaries are the only ordering between the workgroups; the walk over the owned slots is slot_walk.hpp's.  Every
// sum is of integers and every other word one fp32 value with a fixed operand order: the same bytes from run to run.
//
// d2 is never fused: the files are built with -ffp-contract=off, and the gfx950 ISA of both walk kernels holds no floating-point
// fma, mad or fmac of any kind -- the differences are v_pk_add_f32 with a negated operand, the squares v_pk_mul_f32, the sums
// v_pk_add_f32 (the only mads are the 64-bit integer ones of the address arithmetic).
//
// VGPRs / waves per SIMD as the compiler reports them for gfx950, no kernel with scratch:
//   k_nbr_count 28 / 8      k_nbr_fill 26 / 8      k_nbr_reduce 42 / 8      k_nbr_index 25 / 7 (106 SGPRs)      k_nbr_finish 85 / 5
#include "nbr_walk.hpp"
#include "slot_walk.hpp"

namespace psamd {

constexpr int NBR_THREADS = SLOT_THREADS, NBR_WAVES = SLOT_WAVES, NBR_ITEMS = SLOT_ITEMS;
constexpr float NBR_INF = __builtin_huge_valf();

// the count pass's view of a task: per lane the count and the nearest pair, ties to the lower global slot id
struct NbrCount {
    int *cnt_sorted, *who_sorted;
    float *d2_sorted;
    int n, who;
    float best;
    __device__ __forceinline__ void begin(int, bool) { n = 0; who = -1; best = NBR_INF; }
    __device__ __forceinline__ void operator()(bool hit, int id, float d2)
    {
        n += hit ? 1 : 0;
        const bool better = hit && (d2 < best || (d2 == best && id < who));
        best = better ? d2 : best;
        who = better ? id : who;
    }
    __device__ __forceinline__ void end(int gi, bool valid)
    {
        if (valid) { cnt_sorted[gi] = n; who_sorted[gi] = who; d2_sorted[gi] = best; }
    }
};

__global__ __launch_bounds__(NBR_THREADS) void k_nbr_count(DevParams P, const int *__restrict__ cell_start,
                                                           const float *__restrict__ snap_soa, const float *__restrict__ snap_age,
                                                           const int *__restrict__ sorted_id, const float4 *__restrict__ pos4,
                                                           float r2, int *__restrict__ cnt_sorted, int *__restrict__ who_sorted,
                                                           float *__restrict__ d2_sorted)
{
    NbrCount f{cnt_sorted, who_sorted, d2_sorted, 0, -1, NBR_INF};
    nbr_walk_task(P, cell_start, snap_soa, snap_age, sorted_id, pos4, r2, f);
}

// the fill pass's: per lane the running position in the lists; a name goes through the export index table (INDEX) or is the id
struct NbrFill {
    const DevParams &P;
    const int *sorted_id, *index;
    const long long *start;
    int *list;
    long long cap, at;
    __device__ __forceinline__ void begin(int gi, bool valid)
    {
        at = cap;                                    // nothing to store: no query, or an entry past the capacity
        if (valid) {
            const int si = slot_index(P, sorted_id[gi]);
            const long long s = si >= 0 ? start[si] : -1;
            if (s >= 0) at = s;
        }
    }
    __device__ __forceinline__ void operator()(bool hit, int id, float)
    {
        if (hit) {
            if (at < cap) {
                int name = id;
                if (index) { const int sj = slot_index(P, id); name = sj >= 0 ? index[sj] : -1; }
                list[at] = name;
            }
            at++;
        }
    }
    __device__ __forceinline__ void end(int, bool) {}
};

__global__ __launch_bounds__(NBR_THREADS) void k_nbr_fill(DevParams P, const int *__restrict__ cell_start,
                                                          const float *__restrict__ snap_soa, const float *__restrict__ snap_age,
                                                          const int *__restrict__ sorted_id, const float4 *__restrict__ pos4,
                                                          float r2, const int *__restrict__ index,
                                                          const long long *__restrict__ start, int *__restrict__ list,
                                                          long long list_capacity)
{
    NbrFill f{P, sorted_id, index, start, list, list_capacity, list_capacity};
    nbr_walk_task(P, cell_start, snap_soa, snap_age, sorted_id, pos4, r2, f);
}

// What a tile, a wave or a lane has seen of the queries.
struct NbrAcc {
    long long pairs;
    float d2_min;
    int listed, max_count;
    __device__ __forceinline__ void init() { pairs = 0; d2_min = NBR_INF; listed = 0; max_count = 0; }
    __device__ __forceinline__ void add(int n, float d2) { listed++; pairs += n; max_count = max(max_count, n); d2_min = fminf(d2_min, d2); }
    __device__ __forceinline__ void merge(const NbrAcc &o)
    {
        pairs += o.pairs; d2_min = fminf(d2_min, o.d2_min); listed += o.listed; max_count = max(max_count, o.max_count);
    }
    __device__ __forceinline__ void wave_reduce()
    {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            NbrAcc o;
            o.pairs = __shfl_xor(pairs, m); o.d2_min = __shfl_xor(d2_min, m);
            o.listed = __shfl_xor(listed, m); o.max_count = __shfl_xor(max_count, m);
            merge(o);
        }
    }
};

__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// Tile t of the sorted order of the own cells (an entry whose id is -1 was ranked past its cell's list capacity: no particle)
// and tile t of the owned slots (k_pot_reduce's pairing).
__global__ __launch_bounds__(NBR_THREADS) void k_nbr_reduce(DevParams P, const int *__restrict__ cell_start,
                                                            const int *__restrict__ sorted_id, const int *__restrict__ cell,
                                                            const NbrScratch s)
{
    __shared__ NbrAcc s_acc[NBR_WAVES];
    __shared__ int s_live[NBR_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x;
    const int g0 = cell_start[0], g1 = min(cell_start[P.n_own_cells], P.sorted_cap);
    const int off = t * SLOT_TILE + wv * 64 * NBR_ITEMS + lane;
    NbrAcc a;
    a.init();
    int live = 0;
#pragma unroll 4
    for (int k = 0; k < NBR_ITEMS; k++) {
        const int gi = g0 + off + 64 * k;
        const int id = gi < g1 ? sorted_id[gi] : -1;
        if (id >= 0) {
            const int n = s.cnt_sorted[gi], who = s.who_sorted[gi];
            const float d2 = s.d2_sorted[gi];
            a.add(n, d2);
            const int si = slot_index(P, id);
            if (si >= 0) { s.cnt_slot[si] = n; s.who_slot[si] = who; s.d2_slot[si] = d2; }
        }
        live += __popcll(__ballot(slot_live(P, slot_cell(P, cell, off + 64 * k))));
    }
    a.wave_reduce();
    if (lane == 0) { s_acc[wv] = a; s_live[wv] = live; }
    __syncthreads();
    if (threadIdx.x == 0) {
        NbrAcc b = s_acc[0];
        int n = s_live[0];
        for (int w = 1; w < NBR_WAVES; w++) { b.merge(s_acc[w]); n += s_live[w]; }
        NbrTile &r = s.tiles[t];
        r.pairs = b.pairs; r.d2_min = b.d2_min; r.listed = b.listed; r.max_count = b.max_count; r.pad = 0;
        s.tile_live[t] = n;
    }
}

// Slot tile t: every live slot's export index (the walk of k_export_write), and the counts of its entries below the capacity.
__global__ __launch_bounds__(NBR_THREADS) void k_nbr_index(DevParams P, const int *__restrict__ cell, long long capacity,
                                                           const NbrScratch s)
{
    __shared__ long long s_sum[NBR_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x;
    const int before = tiles_before(s.tile_live, t);
    const int first = slot_first(t, wv, lane);
    unsigned long long mask[NBR_ITEMS];
    int live = 0;
#pragma unroll
    for (int k = 0; k < NBR_ITEMS; k++) {
        mask[k] = __ballot(slot_live(P, slot_cell(P, cell, first + 64 * k)));
        live += __popcll(mask[k]);
    }
    long long at = wave_offset<long long>(before, live, wv, lane);
    long long sum = 0;
#pragma unroll
    for (int k = 0; k < NBR_ITEMS; k++) {
        const unsigned long long m = mask[k];
        const long long o = at + (long long)lane_rank(m);
        at += __popcll(m);
        const int si = first + 64 * k;
        if (si < P.slots_total) {
            const bool is = (m >> lane) & 1ull;
            s.index[si] = is ? (int)o : -1;
            if (is && o < capacity) sum += max(s.cnt_slot[si], 0);
        }
    }
    sum = wave_sum(sum);
    if (lane == 0) s_sum[wv] = sum;
    __syncthreads();
    if (threadIdx.x == 0) s.tile_sum[t] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}
static_assert(NBR_WAVES == 4, "k_nbr_index and k_nbr_finish add four waves' words");

// Workgroup 0: the record over the tiles -- integers, a minimum and a maximum: any tree gives the same answer -- and
// offsets[m], m = min(live, capacity).
__device__ __forceinline__ void nbr_finish_record(int ntiles, long long capacity, const NbrScratch &s, long long *__restrict__ offsets,
                                                  psamd_neighbours_result *__restrict__ result_out)
{
    __shared__ NbrAcc s_acc[NBR_WAVES];
    __shared__ long long s_word[3][NBR_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    NbrAcc a;
    a.init();
    long long listed = 0, live = 0, want = 0;
    for (int t = tid; t < ntiles; t += NBR_THREADS) {
        const NbrTile r = s.tiles[t];
        a.pairs += r.pairs; a.d2_min = fminf(a.d2_min, r.d2_min); a.max_count = max(a.max_count, r.max_count);
        listed += r.listed; live += s.tile_live[t]; want += s.tile_sum[t];
    }
    a.wave_reduce();
    listed = wave_sum(listed); live = wave_sum(live); want = wave_sum(want);
    if (lane == 0) { s_acc[wv] = a; s_word[0][wv] = listed; s_word[1][wv] = live; s_word[2][wv] = want; }
    __syncthreads();
    if (tid == 0) {
        NbrAcc b = s_acc[0];
        for (int w = 1; w < NBR_WAVES; w++) b.merge(s_acc[w]);
        long long v[3];
        for (int k = 0; k < 3; k++) v[k] = s_word[k][0] + s_word[k][1] + s_word[k][2] + s_word[k][3];
        psamd_neighbours_result r;
        r.listed = v[0]; r.pairs = b.pairs; r.wanted = v[2]; r.max_count = b.max_count; r.reserved = 0; r.d2_min = (double)b.d2_min;
        s.own->result = r; s.own->live = v[1];
        if (result_out) *result_out = r;
        if (offsets) offsets[min(v[1], capacity)] = v[2];
    }
}

// Workgroup 1 + t: slot tile t to export order.  A slot's entry is where k_nbr_index put it; offsets run on from the sums of
// the tiles before, wave by wave, batch by batch, lane by lane -- the slot order.
__global__ __launch_bounds__(NBR_THREADS) void k_nbr_finish(DevParams P, int ntiles, NbrArgs a, const NbrScratch s)
{
    long long *offsets = reinterpret_cast<long long *>(a.offsets);
    if (blockIdx.x == 0) { nbr_finish_record(ntiles, a.capacity, s, offsets, a.result); return; }
    __shared__ long long s_base[NBR_WAVES];
    __shared__ int s_wave[NBR_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x - 1;
    long long base = 0;
    for (int i = threadIdx.x; i < t; i += NBR_THREADS) base += s.tile_sum[i];
    base = wave_sum(base);
    const int first = slot_first(t, wv, lane);
    int idx[NBR_ITEMS], cnt[NBR_ITEMS], mine = 0;
#pragma unroll
    for (int k = 0; k < NBR_ITEMS; k++) {
        const int si = first + 64 * k;
        idx[k] = -1; cnt[k] = -1;
        if (si < P.slots_total) {
            const int o = s.index[si];
            if (o >= 0 && o < a.capacity) { idx[k] = o; cnt[k] = s.cnt_slot[si]; }
        }
        mine += max(cnt[k], 0);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m);
    if (lane == 0) { s_base[wv] = base; s_wave[wv] = mine; }
    __syncthreads();
    long long at = s_base[0] + s_base[1] + s_base[2] + s_base[3];
    for (int w = 0; w < wv; w++) at += s_wave[w];
    const bool by_index = (a.flags & PSAMD_NEIGHBOURS_INDEX) != 0;
#pragma unroll
    for (int k = 0; k < NBR_ITEMS; k++) {
        const int si = first + 64 * k, v = max(cnt[k], 0);
        const int incl = wave_incl_scan(v);
        const long long off = at + (incl - v);
        at += __builtin_amdgcn_readlane(incl, 63);
        if (si >= P.slots_total) continue;
        s.start[si] = idx[k] >= 0 ? off : -1;
        if (idx[k] < 0) continue;
        const int o = idx[k];
        if (a.count) a.count[o] = cnt[k];
        if (offsets) offsets[o] = off;
        if (a.nearest || a.nearest_d2) {
            int who = -1;
            float d2 = NBR_INF;
            if (cnt[k] > 0) {
                who = s.who_slot[si]; d2 = s.d2_slot[si];
                if (by_index) { const int sj = slot_index(P, who); who = sj >= 0 ? s.index[sj] : -1; }
            }
            if (a.nearest) a.nearest[o] = who;
            if (a.nearest_d2) a.nearest_d2[o] = d2;
        }
    }
}

// the one allocation, carved: 8-byte words first
static size_t nbr_carve(const DevParams &P, char *b, NbrScratch *s)
{
    const size_t C = (size_t)std::max(P.slots_total, 1), SC = (size_t)P.sorted_cap + 64, T = (size_t)std::max(slot_tiles(P.slots_total), 1);
    size_t at = 0;
    const auto take = [&](auto *&p, size_t n) {
        using W = std::remove_reference_t<decltype(*p)>;
        if (s) p = reinterpret_cast<W *>(b + at);
        at += (n * sizeof(W) + 255) / 256 * 256;
    };
    NbrScratch dummy{};
    NbrScratch &r = s ? *s : dummy;
    take(r.own, 1); take(r.start, C); take(r.tile_sum, T); take(r.tiles, T);
    take(r.cnt_sorted, SC); take(r.who_sorted, SC); take(r.d2_sorted, SC);
    take(r.cnt_slot, C); take(r.who_slot, C); take(r.d2_slot, C); take(r.index, C); take(r.tile_live, T);
    return at;
}

size_t neighbours_scratch_bytes(const DevParams &P) { return nbr_carve(P, nullptr, nullptr); }

void neighbours_scratch_carve(const DevParams &P, void *block, NbrScratch &s)
{
    s.block = block;
    (void)nbr_carve(P, static_cast<char *>(block), &s);
}

hipError_t launch_neighbours(hipStream_t st, const DevParams &P, const DeviceState &d, const NbrArgs &a, const NbrScratch &s)
{
    const int ntiles = slot_tiles(P.slots_total);
    const int ntask = P.n_own_cells * P.slices;
    // a live particle that is in no list of the frame keeps this -1
    if (ntiles > 0) { const hipError_t e = launch_fill_int(st, s.cnt_slot, -1, (size_t)P.slots_total); if (e != hipSuccess) return e; }
    if (ntask > 0) {
        k_nbr_count<<<(ntask + 3) / 4, NBR_THREADS, 0, st>>>(P, d.cell_start, d.snap_soa, d.snap_age, d.sorted_id, d.pos4, a.r2,
                                                             s.cnt_sorted, s.who_sorted, s.d2_sorted);
        PS_LAUNCH_CHECK();
    }
    if (ntiles > 0) {
        k_nbr_reduce<<<ntiles, NBR_THREADS, 0, st>>>(P, d.cell_start, d.sorted_id, d.cell, s);
        PS_LAUNCH_CHECK();
        k_nbr_index<<<ntiles, NBR_THREADS, 0, st>>>(P, d.cell, (long long)a.capacity, s);
        PS_LAUNCH_CHECK();
    }
    const bool arrays = ntiles > 0 && a.capacity > 0 && (a.count || a.nearest || a.nearest_d2 || a.offsets);
    k_nbr_finish<<<arrays ? ntiles + 1 : 1, NBR_THREADS, 0, st>>>(P, ntiles, a, s);
    PS_LAUNCH_CHECK();
    if (arrays && a.list && a.list_capacity > 0 && ntask > 0) {
        k_nbr_fill<<<(ntask + 3) / 4, NBR_THREADS, 0, st>>>(P, d.cell_start, d.snap_soa, d.snap_age, d.sorted_id, d.pos4, a.r2,
                                                            (a.flags & PSAMD_NEIGHBOURS_INDEX) ? s.index : nullptr, s.start, a.list,
                                                            (long long)a.list_capacity);
        PS_LAUNCH_CHECK();
    }
    return hipSuccess;
}

}  // namespace psamd
