// groups.hip -- psamd_groups: the friends-of-friends groups of the listed particles, the connected components of
// psamd_neighbours' "within a radius" relation, on the device and without a pair list.
//
// Not part of the step and not in the reference.  The pass reads the frame psamd_build_grid left and walks psamd_neighbours'
// tasks with its walk (nbr_walk.hpp, used as it is: the members are the walk's queries that are no kids, which the functor's
// begin sees from snap_age, so the walk needed no flag).  include/psamd.h, "groups within a radius", holds the definition.
// Five launches that nothing in between has to wait for -- the launch boundaries are the only ordering:
//   k_grp_init     parent[si] = si, member[si] = size[si] = 0 over the owned slots; the two counters to 0.
//   k_grp_hook     the walk: a lane marks its query a member; per hit with a candidate of a LOWER storage index (the relation
//                  is symmetric bit for bit, so every undirected link is met exactly once this way, and counted there) the
//                  union of the two slots.
//   k_grp_roots    per tile of slots: root[si] = find(si), read-only on parent; a member adds 1 to size[root] (integer
//                  atomicAdd, a wave's members of its first member's set as one add); the tile's live slots, members and
//                  roots.  (Flattening and sizing share the launch: size[] is read behind the next boundary only.)
//   k_grp_number   per tile of slots: the slot -> export index table and the roots' dense numbers (two exclusive scans over
//                  slot_walk.hpp's tile walk), the two tables; the tile's singles and largest set.
//   k_grp_finish   workgroup 0: the record over the tiles; workgroup 1 + t: group[] of slot tile t in export order.
//
// Why no loop here can spin.  The union-find is over storage indices and a set's root is its smallest slot.
//   (1) A parent word is written by k_grp_init (parent[si] = si) and from then on by atomicMin alone -- the hook, the retry
//       and the path halving -- with a value that is a smaller slot of the same group.  So a word never rises, parent[x] <= x
//       always, and whatever a lane reads of it, however stale, is x itself or a smaller slot of x's group.
//   (2) grp_union keeps the pair (hi, lo), hi > lo.  A step reads p = parent[hi]; if p < hi it goes on with {p, lo}; else it
//       tries old = atomicMin(&parent[hi], lo) and is done if old == hi (hi was a root and hangs under lo now), else goes on
//       with {old, lo}, old < hi.  Every step replaces the pair's LARGER slot by a strictly smaller one: max(hi, lo) falls by
//       at least 1 per step whatever other waves do, and it starts below slots_total and cannot fall below 0.  A union
//       therefore ends in fewer than slots_total steps by itself; find (k_grp_roots) walks x -> parent[x] < x and ends alike.
//   (3) No lock, no wait on a word another thread must write, no grid barrier, no cooperative launch.
//   (4) On top of that every union counts its steps and stops at slots_total, adding 1 to `unfinished`; a word outside
//       [0, slots_total) stops it too.  By (2) correct code never gets there: the cap turns a bug into a failing assertion
//       (unfinished == 0 in every test), not into a hang.
// Stale reads cost steps, not correctness: the atomicMin returns the word's true value, and a union is done only when it saw
// hi == lo or hooked a true root.
//
// Every output word is an integer that depends on the frame and the radius alone -- the components, their smallest slots,
// counts, a maximum and sums: the hooking order does not enter, the bytes are the same from run to run.  There is no
// floating-point atomic; d2 is nbr_walk.hpp's, never fused (-ffp-contract=off).
//
// VGPRs / waves per SIMD as the compiler reports them for gfx950, no kernel with scratch:
//   k_grp_init 8 / 8      k_grp_hook 24 / 7 (106 SGPRs)      k_grp_roots 16 / 8      k_grp_number 48 / 7 (106 SGPRs)      k_grp_finish 29 / 8
#include "nbr_walk.hpp"
#include "slot_walk.hpp"

namespace psamd {

constexpr int GRP_THREADS = SLOT_THREADS, GRP_WAVES = SLOT_WAVES, GRP_ITEMS = SLOT_ITEMS;
static_assert(GRP_WAVES == 4, "the tile kernels add four waves' words");

__device__ __forceinline__ int grp_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The union of the sets of slots a and b (the header's (2)); false: the cap was hit, or a word was no slot.
__device__ __forceinline__ bool grp_union(int *__restrict__ parent, int a, int b, int slots)
{
    int hi = max(a, b), lo = min(a, b);
    for (int step = 0; step < slots; step++) {
        if (hi == lo) return true;
        int p = grp_load(parent + hi);
        if (p >= hi) {                                 // a root as far as this lane sees: hang it under lo
            p = atomicMin(parent + hi, lo);
            if (p >= hi) return p == hi;
        } else if (p >= 0) {                           // path halving: hi's word falls to its grandparent
            const int gp = grp_load(parent + p);
            if (gp >= 0 && gp < p) { atomicMin(parent + hi, gp); p = gp; }
        }
        if (p < 0) return false;
        hi = max(p, lo); lo = min(p, lo);              // (p < the old hi, lo < the old hi)
    }
    return hi == lo;
}

// the set's smallest slot; x falls at every step, so the loop ends by itself
__device__ __forceinline__ int grp_find(const int *__restrict__ parent, int x)
{
    for (;;) {
        const int p = parent[x];
        if (p >= x || p < 0) return x;
        x = p;
    }
}

__global__ __launch_bounds__(GRP_THREADS) void k_grp_init(int slots, const GrpScratch s)
{
    for (int si = blockIdx.x * GRP_THREADS + threadIdx.x; si < slots; si += gridDim.x * GRP_THREADS) {
        s.parent[si] = si; s.member[si] = 0; s.size[si] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { *s.links = 0ull; *s.unfinished = 0; }
}

// the hooking pass's view of a task: per lane its query's storage index (-1: no member) and the links it counted
struct GrpHook {
    const DevParams &P;
    const int *sorted_id;
    const float *snap_age;
    const GrpScratch &s;
    int si, n;
    __device__ __forceinline__ void begin(int gi, bool valid)
    {
        si = -1; n = 0;
        if (valid && !(snap_age[gi] < P.kid_thr)) {    // the walk's own test of a candidate: a kid is no member
            const int id = sorted_id[gi];
            si = id >= 0 ? slot_index(P, id) : -1;
            if (si >= 0) s.member[si] = 1;
        }
    }
    __device__ __forceinline__ void operator()(bool hit, int id, float)
    {
        if (hit && si >= 0) {
            const int sj = slot_index(P, id);
            if (sj >= 0 && sj < si) {                  // the pair's other side skips it: sj > si there
                n++;
                if (!grp_union(s.parent, si, sj, P.slots_total)) atomicAdd(s.unfinished, 1);
            }
        }
    }
    __device__ __forceinline__ void end(int, bool)
    {
        int v = n;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        if ((threadIdx.x & 63) == 0 && v > 0) atomicAdd(s.links, (unsigned long long)v);
    }
};

__global__ __launch_bounds__(GRP_THREADS) void k_grp_hook(DevParams P, const int *__restrict__ cell_start,
                                                          const float *__restrict__ snap_soa, const float *__restrict__ snap_age,
                                                          const int *__restrict__ sorted_id, const float4 *__restrict__ pos4,
                                                          float r2, const GrpScratch s)
{
    GrpHook f{P, sorted_id, snap_age, s, -1, 0};
    nbr_walk_task(P, cell_start, snap_soa, snap_age, sorted_id, pos4, r2, f);
}

// Slot tile t: every slot's root, the sizes at the roots, the tile's counts.
__global__ __launch_bounds__(GRP_THREADS) void k_grp_roots(DevParams P, const int *__restrict__ cell, const GrpScratch s)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x;
    const int first = slot_first(t, wv, lane);
    int live = 0, members = 0, roots = 0;
#pragma unroll 2
    for (int k = 0; k < GRP_ITEMS; k++) {
        const int si = first + 64 * k;
        const bool in = si < P.slots_total;
        const int r = in ? grp_find(s.parent, si) : -1;
        const bool mem = in && s.member[si] != 0;
        if (in) s.root[si] = r;
        live += __popcll(__ballot(slot_live(P, slot_cell(P, cell, si))));
        const unsigned long long mm = __ballot(mem);
        members += __popcll(mm);
        roots += __popcll(__ballot(mem && r == si));
        if (mm) {                                      // the members of the first member's set as one add, the others one each
            const int lead = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(mm));
            const int r0 = __builtin_amdgcn_readlane(r, lead);
            const unsigned long long same = __ballot(mem && r == r0);
            if (lane == lead) atomicAdd(s.size + r0, __popcll(same));
            else if (mem && r != r0) atomicAdd(s.size + r, 1);
        }
    }
    __shared__ int s_w[3][GRP_WAVES];
    if (lane == 0) { s_w[0][wv] = live; s_w[1][wv] = members; s_w[2][wv] = roots; }
    __syncthreads();
    if (threadIdx.x == 0) {
        GrpTile &o = s.tiles[t];
        o.live = s_w[0][0] + s_w[0][1] + s_w[0][2] + s_w[0][3];
        o.members = s_w[1][0] + s_w[1][1] + s_w[1][2] + s_w[1][3];
        o.roots = s_w[2][0] + s_w[2][1] + s_w[2][2] + s_w[2][3];
    }
}

// Slot tile t: the export indices (the walk of k_export_write) and the roots' numbers in slot order; a root writes its group's
// entry of the two tables.
__global__ __launch_bounds__(GRP_THREADS) void k_grp_number(DevParams P, const int *__restrict__ cell, GrpArgs a, const GrpScratch s)
{
    __shared__ int s_before[2][GRP_WAVES], s_n[2][GRP_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x;
    int before[2] = {0, 0};
    for (int i = threadIdx.x; i < t; i += GRP_THREADS) { before[0] += s.tiles[i].live; before[1] += s.tiles[i].roots; }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { before[0] += __shfl_xor(before[0], m); before[1] += __shfl_xor(before[1], m); }
    const int first = slot_first(t, wv, lane);
    unsigned long long live_m[GRP_ITEMS], root_m[GRP_ITEMS];
    int n[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < GRP_ITEMS; k++) {
        const int si = first + 64 * k;
        live_m[k] = __ballot(slot_live(P, slot_cell(P, cell, si)));
        root_m[k] = __ballot(si < P.slots_total && s.member[si] != 0 && s.root[si] == si);
        n[0] += __popcll(live_m[k]); n[1] += __popcll(root_m[k]);
    }
    if (lane == 0) { s_before[0][wv] = before[0]; s_before[1][wv] = before[1]; s_n[0][wv] = n[0]; s_n[1][wv] = n[1]; }
    __syncthreads();
    int at[2] = {0, 0};
    for (int w = 0; w < GRP_WAVES; w++)
        for (int j = 0; j < 2; j++) at[j] += s_before[j][w] + (w < wv ? s_n[j][w] : 0);
    const bool by_index = (a.flags & PSAMD_GROUPS_INDEX) != 0;
    int singles = 0, largest = 0;
#pragma unroll
    for (int k = 0; k < GRP_ITEMS; k++) {
        const int si = first + 64 * k;
        const bool is_live = (live_m[k] >> lane) & 1ull, is_root = (root_m[k] >> lane) & 1ull;
        const int o = at[0] + lane_rank(live_m[k]), g = at[1] + lane_rank(root_m[k]);
        at[0] += __popcll(live_m[k]); at[1] += __popcll(root_m[k]);
        if (si >= P.slots_total) continue;
        s.index[si] = is_live ? o : -1;
        if (!is_root) continue;
        const int size = s.size[si];
        s.number[si] = g;
        singles += size == 1 ? 1 : 0;
        largest = max(largest, size);
        if (g < a.group_capacity) {
            if (a.group_first) a.group_first[g] = by_index ? (is_live ? o : -1) : slot_of_index(P, si);
            if (a.group_size) a.group_size[g] = size;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { singles += __shfl_xor(singles, m); largest = max(largest, __shfl_xor(largest, m)); }
    __shared__ int s_w[2][GRP_WAVES];
    if (lane == 0) { s_w[0][wv] = singles; s_w[1][wv] = largest; }
    __syncthreads();
    if (threadIdx.x == 0) {                            // (the tile's other words are k_grp_roots')
        GrpTile &o = s.tiles[t];
        o.singles = s_w[0][0] + s_w[0][1] + s_w[0][2] + s_w[0][3];
        o.largest = max(max(s_w[1][0], s_w[1][1]), max(s_w[1][2], s_w[1][3]));
    }
}

// Workgroup 0: the record over the tiles -- integers, a maximum and sums: any tree gives the same words.
__device__ __forceinline__ void grp_finish_record(int ntiles, const GrpScratch &s, psamd_groups_result *__restrict__ result_out)
{
    __shared__ long long s_word[5][GRP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    long long v[5] = {0, 0, 0, 0, 0};                  // live, members, roots, singles, largest
    for (int t = tid; t < ntiles; t += GRP_THREADS) {
        const GrpTile r = s.tiles[t];
        v[0] += r.live; v[1] += r.members; v[2] += r.roots; v[3] += r.singles; v[4] = max(v[4], (long long)r.largest);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        for (int k = 0; k < 4; k++) v[k] += __shfl_xor(v[k], m);
        v[4] = max(v[4], __shfl_xor(v[4], m));
    }
    if (lane == 0) for (int k = 0; k < 5; k++) s_word[k][wv] = v[k];
    __syncthreads();
    if (tid == 0) {
        for (int k = 0; k < 4; k++) v[k] = s_word[k][0] + s_word[k][1] + s_word[k][2] + s_word[k][3];
        v[4] = max(max(s_word[4][0], s_word[4][1]), max(s_word[4][2], s_word[4][3]));
        psamd_groups_result r;
        r.members = v[1]; r.groups = v[2]; r.links = (long long)*s.links; r.singles = v[3]; r.largest = (int)v[4]; r.unfinished = *s.unfinished;
        s.own->result = r; s.own->live = v[0];
        if (result_out) *result_out = r;
    }
}

// Workgroup 1 + t: slot tile t's entries of group[], where k_grp_number put them in the export order.
__global__ __launch_bounds__(GRP_THREADS) void k_grp_finish(DevParams P, int ntiles, GrpArgs a, const GrpScratch s)
{
    if (blockIdx.x == 0) { grp_finish_record(ntiles, s, a.result); return; }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x - 1;
    const int first = slot_first(t, wv, lane);
#pragma unroll 4
    for (int k = 0; k < GRP_ITEMS; k++) {
        const int si = first + 64 * k;
        if (si >= P.slots_total) continue;
        const int o = s.index[si];
        if (o < 0 || o >= a.capacity) continue;
        a.group[o] = s.member[si] != 0 ? s.number[s.root[si]] : -1;
    }
}

// the one allocation, carved: 8-byte words first
static size_t grp_carve(const DevParams &P, char *b, GrpScratch *s)
{
    const size_t C = (size_t)std::max(P.slots_total, 1), T = (size_t)std::max(slot_tiles(P.slots_total), 1);
    size_t at = 0;
    const auto take = [&](auto *&p, size_t n) {
        using W = std::remove_reference_t<decltype(*p)>;
        if (s) p = reinterpret_cast<W *>(b + at);
        at += (n * sizeof(W) + 255) / 256 * 256;
    };
    GrpScratch dummy{};
    GrpScratch &r = s ? *s : dummy;
    take(r.own, 1); take(r.links, 1); take(r.tiles, T);
    take(r.parent, C); take(r.member, C); take(r.root, C); take(r.size, C); take(r.number, C); take(r.index, C); take(r.unfinished, 1);
    return at;
}

size_t groups_scratch_bytes(const DevParams &P) { return grp_carve(P, nullptr, nullptr); }

void groups_scratch_carve(const DevParams &P, void *block, GrpScratch &s)
{
    s.block = block;
    (void)grp_carve(P, static_cast<char *>(block), &s);
}

hipError_t launch_groups(hipStream_t st, const DevParams &P, const DeviceState &d, const GrpArgs &a, const GrpScratch &s)
{
    const int ntiles = slot_tiles(P.slots_total);
    const int ntask = P.n_own_cells * P.slices;
    k_grp_init<<<std::max(blocks_for((size_t)P.slots_total, GRP_THREADS), 1), GRP_THREADS, 0, st>>>(P.slots_total, s);
    PS_LAUNCH_CHECK();
    if (ntask > 0 && ntiles > 0) {
        k_grp_hook<<<(ntask + 3) / 4, GRP_THREADS, 0, st>>>(P, d.cell_start, d.snap_soa, d.snap_age, d.sorted_id, d.pos4, a.r2, s);
        PS_LAUNCH_CHECK();
    }
    if (ntiles > 0) {
        k_grp_roots<<<ntiles, GRP_THREADS, 0, st>>>(P, d.cell, s);
        PS_LAUNCH_CHECK();
        k_grp_number<<<ntiles, GRP_THREADS, 0, st>>>(P, d.cell, a, s);
        PS_LAUNCH_CHECK();
    }
    const bool arrays = ntiles > 0 && a.capacity > 0 && a.group;
    k_grp_finish<<<arrays ? ntiles + 1 : 1, GRP_THREADS, 0, st>>>(P, ntiles, a, s);
    PS_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace psamd
