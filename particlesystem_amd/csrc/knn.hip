// knn.hip -- psamd_knn: every listed particle's k nearest neighbours within a radius, ordered by (d2, global slot id), on the
// device.
//
// Not part of the step and not in the reference.  The pass reads the frame psamd_build_grid left and walks psamd_neighbours'
// tasks with its walk (nbr_walk.hpp, used as it is); include/psamd.h, "the k nearest within a radius", holds the definition.
// Four launches that nothing in between has to wait for -- the launch boundaries are the only ordering:
//   k_knn_live     per tile of slots: the tile's live slots; and the tasks' partials to "no query".
//   k_knn_index    per tile of slots: the slot -> export index table (the walk of k_nbr_index), and for the entries below the
//                  capacity the default row (-1 / +inf) and found = -1, which a live particle in no list of the frame keeps.
//                  (The table needs every earlier tile's live count, so the count is a launch of its own: one launch for both
//                  would have a tile wait for words other workgroups write, which no kernel here does.)
//   k_knn_walk<K>  the walk: a lane keeps its query's best K by the key in 2 K registers and stores the first k of them
//                  straight to the caller's rows through the table; the wave's found, full, listed and k-th d2 as the task's
//                  partial.  K is the tier, the smallest of 1, 8, 16, 32 that holds k: a k = 7 call does not pay for 32.
//   k_knn_finish   one workgroup: the partials in task order into the record -- integer sums, a minimum and a maximum of fp32
//                  values, any tree gives the same words -- the context's own copy and result_dev.
// The scratch is the table, the tiles' live counts and the tasks' partials: it depends on the container alone, never on k.
//
// The best K.  The row is K (d2, id) pairs in registers that are only ever indexed by unrolled constants (a run-time index
// would put the row in scratch).  Ahead of the insertion stands a reject: a hit whose key is not below the row's last entry is
// dropped (an empty entry is (+inf, -1) and a hit's d2 is finite, so a row that is not full takes every hit).  The candidate is
// the same for all lanes, so "no lane accepts" is a scalar branch around the whole insertion; once the rows have filled almost
// every candidate ends there.  An accepted hit goes in by one unrolled sweep from the tail: position j takes its left
// neighbour's pair where the new key is below that neighbour's, the new pair where it is below its own only, and keeps its pair
// otherwise -- the row is sorted, so these are the three cases, and no index is carried from one position to the next.  Keys
// are distinct (an id stands once in the stencil), so the row is the K smallest hits in ascending order whatever the walk
// order; with K > k its first k words are the k smallest.  With k = 1 the comparison is NbrCount's: psamd_neighbours' nearest
// and nearest_d2, byte for byte.
//
// Row stores.  A lane stores its row's k words one after the other, so across the lanes a store is strided by k words.  That
// is k store instructions of 64 scattered words per task and array against a walk of hundreds of candidate groups: measured on
// the benchmark frame (profiles/knn_cost.txt) the call with found and the rows takes 0.12 ms more than the record alone at
// k = 32 (1.60 against 1.48 ms at radius 1.0) and 0.03 ms or less at k <= 8, so the stores are not transposed through LDS.
//
// Cost (the same file): 0.86 / 0.91 / 1.60 ms at k = 1 / 8 / 32 at radius 1.0, 0.88 / 1.00 / 2.26 ms at cell_size, beside 0.81-0.84
// ms for psamd_neighbours' count-and-offsets call and 1.37-1.39 ms for its with-lists call.  k = 32 is SLOWER than the with-lists
// call: rows of 32 almost never fill on that frame, so the reject never closes and every hit of any lane takes the wave through
// the 32-position sweep (sixteen copies of it are inlined in the walk's unrolled body), at 5 waves per SIMD.
//
// d2 is nbr_walk.hpp's, never fused (-ffp-contract=off); there is no atomic of any kind in this file.
//
// VGPRs / waves per SIMD as the compiler reports them for gfx950, no kernel with scratch:
//   k_knn_live 14 / 8      k_knn_index 23 / 7 (106 SGPRs)      k_knn_finish 26 / 8
//   k_knn_walk<1> 30 / 8      k_knn_walk<8> 46 / 7 (105 SGPRs)      k_knn_walk<16> 61 / 7      k_knn_walk<32> 94 / 5
#include "nbr_walk.hpp"
#include "slot_walk.hpp"

namespace psamd {

constexpr int KNN_THREADS = SLOT_THREADS, KNN_WAVES = SLOT_WAVES, KNN_ITEMS = SLOT_ITEMS;
constexpr float KNN_INF = __builtin_huge_valf();
static_assert(KNN_WAVES == 4, "the tile kernels add four waves' words");

// Slot tile t: its live slots.  And every task's partial to what a task without a query leaves (the walk ends such a task
// before the functor sees it).
__global__ __launch_bounds__(KNN_THREADS) void k_knn_live(DevParams P, const int *__restrict__ cell, int ntask, const KnnScratch s)
{
    __shared__ int s_live[KNN_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x;
    for (int i = blockIdx.x * KNN_THREADS + threadIdx.x; i < ntask; i += gridDim.x * KNN_THREADS)
        s.parts[i] = KnnPart{0, 0, 0, 0, KNN_INF, -KNN_INF, {0.f, 0.f}};
    const int first = slot_first(t, wv, lane);
    int live = 0;
#pragma unroll 4
    for (int k = 0; k < KNN_ITEMS; k++) live += __popcll(__ballot(slot_live(P, slot_cell(P, cell, first + 64 * k))));
    if (lane == 0) s_live[wv] = live;
    __syncthreads();
    if (threadIdx.x == 0) s.tile_live[t] = s_live[0] + s_live[1] + s_live[2] + s_live[3];
}

// Slot tile t: every live slot's export index (the walk of k_export_write), and its entry's default row.
__global__ __launch_bounds__(KNN_THREADS) void k_knn_index(DevParams P, const int *__restrict__ cell, KnnArgs a, const KnnScratch s)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x;
    const int before = tiles_before(s.tile_live, t);
    const int first = slot_first(t, wv, lane);
    unsigned long long mask[KNN_ITEMS];
    int live = 0;
#pragma unroll
    for (int k = 0; k < KNN_ITEMS; k++) {
        mask[k] = __ballot(slot_live(P, slot_cell(P, cell, first + 64 * k)));
        live += __popcll(mask[k]);
    }
    long long at = wave_offset<long long>(before, live, wv, lane);
#pragma unroll
    for (int k = 0; k < KNN_ITEMS; k++) {
        const unsigned long long m = mask[k];
        const long long o = at + (long long)lane_rank(m);
        at += __popcll(m);
        const int si = first + 64 * k;
        if (si >= P.slots_total) continue;
        const bool is = (m >> lane) & 1ull;
        s.index[si] = is ? (int)o : -1;
        if (!is || o >= a.capacity) continue;
        if (a.found) a.found[o] = -1;
        const long long row = o * a.k;
        if (a.who) for (int j = 0; j < a.k; j++) a.who[row + j] = -1;
        if (a.d2) for (int j = 0; j < a.k; j++) a.d2[row + j] = KNN_INF;
    }
}

// the walk's view of a task: per lane its query's hits and the K smallest of them by (d2, id), ascending
template <int K>
struct KnnBest {
    const DevParams &P;
    const int *sorted_id;
    const KnnArgs &a;
    const KnnScratch &s;
    float d[K];
    int w[K];
    int n;
    long long o;                                     // the query's export index; -1: nothing to store

    __device__ __forceinline__ void begin(int gi, bool valid)
    {
#pragma unroll
        for (int j = 0; j < K; j++) { d[j] = KNN_INF; w[j] = -1; }
        n = 0; o = -1;
        if (valid) {
            const int id = sorted_id[gi];
            const int si = id >= 0 ? slot_index(P, id) : -1;
            if (si >= 0) o = s.index[si];
        }
    }

    __device__ __forceinline__ void operator()(bool hit, int id, float d2)
    {
        n += hit ? 1 : 0;
        // NbrCount's comparison against the row's last entry
        const bool accept = hit && (d2 < d[K - 1] || (d2 == d[K - 1] && id < w[K - 1]));
        if (__ballot(accept) == 0ull) return;        // the candidate is the wave's: a scalar branch
        bool below = accept;                         // the new key is below position j's (true at K - 1: it was accepted)
#pragma unroll
        for (int j = K - 1; j >= 0; j--) {
            bool below_left = false;
            if (j > 0) below_left = accept && (d2 < d[j - 1] || (d2 == d[j - 1] && id < w[j - 1]));
            d[j] = below_left ? d[j - 1] : below ? d2 : d[j];
            w[j] = below_left ? w[j - 1] : below ? id : w[j];
            below = below_left;
        }
    }

    __device__ __forceinline__ void end(int, bool valid)
    {
        const int k = a.k;
        const bool query = valid && o >= 0;          // (a valid lane's entry is a particle of the own cells: its slot is live)
        const int found = min(n, k);
        float dk = KNN_INF;                          // the k-th neighbour's d2: position k - 1 by constants
#pragma unroll
        for (int j = 0; j < K; j++) dk = j == k - 1 ? d[j] : dk;
        const bool full = query && n >= k;
        if (query && o < a.capacity) {
            if (a.found) a.found[o] = found;
            const long long row = o * k;
            const bool by_index = (a.flags & PSAMD_KNN_INDEX) != 0;
#pragma unroll
            for (int j = 0; j < K; j++) {
                if (j >= k) continue;                // (a break would keep the loop rolled and the row's index a run-time one)
                if (a.who) {
                    int name = w[j];                 // (-1 past found: the row's empty entries)
                    if (by_index && name >= 0) { const int sj = slot_index(P, name); name = sj >= 0 ? s.index[sj] : -1; }
                    a.who[row + j] = name;
                }
                if (a.d2) a.d2[row + j] = d[j];
            }
        }
        int v_found = query ? found : 0, v_full = full ? 1 : 0, v_listed = query ? 1 : 0;
        float lo = full ? dk : KNN_INF, hi = full ? dk : -KNN_INF;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            v_found += __shfl_xor(v_found, m); v_full += __shfl_xor(v_full, m); v_listed += __shfl_xor(v_listed, m);
            lo = fminf(lo, __shfl_xor(lo, m)); hi = fmaxf(hi, __shfl_xor(hi, m));
        }
        if ((threadIdx.x & 63) == 0) {               // the task's number: nbr_walk_task's
            const int nwg = (P.n_own_cells * P.slices + 3) >> 2;
            const int task = xcd_contiguous(blockIdx.x, nwg) * 4 + (int)(threadIdx.x >> 6);
            s.parts[task] = KnnPart{v_found, v_full, v_listed, 0, lo, hi, {0.f, 0.f}};
        }
    }
};

template <int K>
__global__ __launch_bounds__(KNN_THREADS) void k_knn_walk(DevParams P, const int *__restrict__ cell_start,
                                                          const float *__restrict__ snap_soa, const float *__restrict__ snap_age,
                                                          const int *__restrict__ sorted_id, const float4 *__restrict__ pos4,
                                                          const KnnArgs a, const KnnScratch s)
{
    KnnBest<K> f{P, sorted_id, a, s};
    nbr_walk_task(P, cell_start, snap_soa, snap_age, sorted_id, pos4, a.r2, f);
}

// One workgroup: the record over the tasks' partials and the tiles' live counts.
__global__ __launch_bounds__(KNN_THREADS) void k_knn_finish(int ntask, int ntiles, KnnArgs a, const KnnScratch s)
{
    __shared__ long long s_word[4][KNN_WAVES];
    __shared__ float s_d[2][KNN_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    long long v[4] = {0, 0, 0, 0};                   // found, full, listed, live
    float lo = KNN_INF, hi = -KNN_INF;
    for (int i = tid; i < ntask; i += KNN_THREADS) {
        const KnnPart p = s.parts[i];
        v[0] += p.found; v[1] += p.full; v[2] += p.listed;
        lo = fminf(lo, p.dk_min); hi = fmaxf(hi, p.dk_max);
    }
    for (int t = tid; t < ntiles; t += KNN_THREADS) v[3] += s.tile_live[t];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        for (int k = 0; k < 4; k++) v[k] += __shfl_xor(v[k], m);
        lo = fminf(lo, __shfl_xor(lo, m)); hi = fmaxf(hi, __shfl_xor(hi, m));
    }
    if (lane == 0) { for (int k = 0; k < 4; k++) s_word[k][wv] = v[k]; s_d[0][wv] = lo; s_d[1][wv] = hi; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 0; k < 4; k++) v[k] = s_word[k][0] + s_word[k][1] + s_word[k][2] + s_word[k][3];
        psamd_knn_result r;
        r.listed = v[2]; r.found = v[0]; r.full = v[1]; r.k = a.k; r.reserved = 0;
        r.dk2_min = (double)fminf(fminf(s_d[0][0], s_d[0][1]), fminf(s_d[0][2], s_d[0][3]));
        r.dk2_max = (double)fmaxf(fmaxf(s_d[1][0], s_d[1][1]), fmaxf(s_d[1][2], s_d[1][3]));
        s.own->result = r; s.own->live = v[3];
        if (a.result) *a.result = r;
    }
}

// the one allocation, carved: 16-byte words first
static size_t knn_carve(const DevParams &P, char *b, KnnScratch *s)
{
    const size_t C = (size_t)std::max(P.slots_total, 1), T = (size_t)std::max(slot_tiles(P.slots_total), 1);
    const size_t N = (size_t)std::max(P.n_own_cells * P.slices, 1);
    size_t at = 0;
    const auto take = [&](auto *&p, size_t n) {
        using W = std::remove_reference_t<decltype(*p)>;
        if (s) p = reinterpret_cast<W *>(b + at);
        at += (n * sizeof(W) + 255) / 256 * 256;
    };
    KnnScratch dummy{};
    KnnScratch &r = s ? *s : dummy;
    take(r.parts, N); take(r.own, 1); take(r.index, C); take(r.tile_live, T);
    return at;
}

size_t knn_scratch_bytes(const DevParams &P) { return knn_carve(P, nullptr, nullptr); }

void knn_scratch_carve(const DevParams &P, void *block, KnnScratch &s)
{
    s.block = block;
    (void)knn_carve(P, static_cast<char *>(block), &s);
}

template <int K>
static void knn_walk(hipStream_t st, int ntask, const DevParams &P, const DeviceState &d, const KnnArgs &a, const KnnScratch &s)
{
    k_knn_walk<K><<<(ntask + 3) / 4, KNN_THREADS, 0, st>>>(P, d.cell_start, d.snap_soa, d.snap_age, d.sorted_id, d.pos4, a, s);
}

hipError_t launch_knn(hipStream_t st, const DevParams &P, const DeviceState &d, const KnnArgs &a, const KnnScratch &s)
{
    const int ntiles = slot_tiles(P.slots_total);
    const int ntask = ntiles > 0 ? P.n_own_cells * P.slices : 0;
    if (ntiles > 0) {
        k_knn_live<<<ntiles, KNN_THREADS, 0, st>>>(P, d.cell, ntask, s);
        PS_LAUNCH_CHECK();
        k_knn_index<<<ntiles, KNN_THREADS, 0, st>>>(P, d.cell, a, s);
        PS_LAUNCH_CHECK();
    }
    if (ntask > 0) {
        if (a.k <= 1) knn_walk<1>(st, ntask, P, d, a, s);
        else if (a.k <= 8) knn_walk<8>(st, ntask, P, d, a, s);
        else if (a.k <= 16) knn_walk<16>(st, ntask, P, d, a, s);
        else knn_walk<PSAMD_KNN_MAX_K>(st, ntask, P, d, a, s);
        PS_LAUNCH_CHECK();
    }
    k_knn_finish<<<1, KNN_THREADS, 0, st>>>(ntask, ntiles, a, s);
    PS_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace psamd
