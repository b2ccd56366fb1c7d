// export.hip -- psamd_export_live: the live particles as compact arrays, and their statistics, on the device.
//
// A deterministic stream compaction of the owned slots in slot order, plus a deterministic reduction over the same
// particles, in two launches that nothing in between has to wait for:
//   k_export_count  pass A, one workgroup per tile of SLOT_TILE owned slots: the tile's live count (wave64 ballot +
//                   popcount) and its statistics partials (fp64 sums, fp32 extrema)
//   k_export_write  pass B, workgroup 1 + t for tile t: the tile's output offset (the exclusive prefix of the tile
//                   counts, rebuilt in the workgroup: fewer than 1000 tiles at N = 2^20), a wave's offset inside the
//                   tile, a lane's rank inside the wave (slot_walk.hpp); then the chosen fields, one 16-byte store
//                   per float4.  Workgroup 0 sums the tiles' partials in tile order and writes the count and the
//                   statistics.
// There is no hand-off between the workgroups of one launch (no flag, no ticket, no spin): the launch boundary between
// the passes is the only ordering (a last-arriver ticket on this part cost 7 -> 251 us).
// The launches cover every owned slot (slots_total); no host-side bound of the live count is used for sizing, since
// such a bound can be stale after an upload or a restore.
//
// A rank's storage order is its slot order (kernels_common.hpp, own_local_cell), so the output is in ascending global
// slot id, and slot_of_index gives the global id.
#include "slot_walk.hpp"

namespace psamd {

constexpr int EXPORT_BATCH = 8;                                 // slots per lane whose loads are in flight together

// The statistics of some live particles: every term formed in fp64 from the fp32 fields; a particle whose position or
// velocity is not a finite number is counted and left out of everything else.
struct ExportAcc {
    double sum[EXPORT_SUMS];
    float lo[4], hi[4];
    int nonfinite;

    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int k = 0; k < EXPORT_SUMS; k++) sum[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; k++) { lo[k] = __int_as_float(0x7f800000); hi[k] = -__int_as_float(0x7f800000); }
        nonfinite = 0;
    }
    __device__ __forceinline__ void add(const float4 p, const float4 v)
    {
        if (!finite3(p.x, p.y, p.z) || !finite3(v.x, v.y, v.z)) { nonfinite++; return; }
        const double w = (double)p.w, vx = (double)v.x, vy = (double)v.y, vz = (double)v.z;
        sum[0] += w;
        sum[1] += w * vx; sum[2] += w * vy; sum[3] += w * vz;
        sum[4] += 0.5 * w * (vx * vx + vy * vy + vz * vz);
        sum[5] += w * (double)p.x; sum[6] += w * (double)p.y; sum[7] += w * (double)p.z;
        sum[8] += (double)v.w;
        lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z); lo[3] = fminf(lo[3], v.w);
        hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z); hi[3] = fmaxf(hi[3], v.w);
    }
    // across the wave: a butterfly, the same fixed tree on every run
    __device__ __forceinline__ void wave_reduce()
    {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
            for (int k = 0; k < EXPORT_SUMS; k++) sum[k] += __shfl_xor(sum[k], m);
#pragma unroll
            for (int k = 0; k < 4; k++) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], m)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], m)); }
            nonfinite += __shfl_xor(nonfinite, m);
        }
    }
};

// Pass A.  Wave w of tile t walks the slots [t * SLOT_TILE + w * 64 * SLOT_ITEMS, + 64 * SLOT_ITEMS), 64 at a
// time; a lane sums its own slots in order, then the wave's butterfly, then the waves in order.
__global__ __launch_bounds__(SLOT_THREADS) void k_export_count(DevParams P, const int *__restrict__ cell,
                                                               const float4 *__restrict__ pos4,
                                                               const float4 *__restrict__ vel4,
                                                               int *__restrict__ tile_count,
                                                               ExportTile *__restrict__ tiles)
{
    __shared__ ExportAcc s_acc[SLOT_WAVES];
    __shared__ int s_live[SLOT_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x;
    const int first = slot_first(t, wv, lane);
    int c[SLOT_ITEMS];
#pragma unroll
    for (int k = 0; k < SLOT_ITEMS; k++) c[k] = slot_cell(P, cell, first + 64 * k);
    ExportAcc a;
    a.init();
    int live = 0;
    // the loads of a batch are issued together, then summed in slot order
#pragma unroll
    for (int k0 = 0; k0 < SLOT_ITEMS; k0 += EXPORT_BATCH) {
        float4 p[EXPORT_BATCH], v[EXPORT_BATCH];
#pragma unroll
        for (int k = 0; k < EXPORT_BATCH; k++) {
            const int i = first + 64 * (k0 + k);
            if (slot_live(P, c[k0 + k])) { p[k] = pos4[i]; v[k] = vel4[i]; }
        }
#pragma unroll
        for (int k = 0; k < EXPORT_BATCH; k++) {
            const bool on = slot_live(P, c[k0 + k]);
            live += __popcll(__ballot(on));
            if (on) a.add(p[k], v[k]);
        }
    }
    a.wave_reduce();
    if (lane == 0) { s_acc[wv] = a; s_live[wv] = live; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ExportAcc b = s_acc[0];
        int n = s_live[0];
        for (int w = 1; w < SLOT_WAVES; w++) {
            const ExportAcc &o = s_acc[w];
#pragma unroll
            for (int k = 0; k < EXPORT_SUMS; k++) b.sum[k] += o.sum[k];
#pragma unroll
            for (int k = 0; k < 4; k++) { b.lo[k] = fminf(b.lo[k], o.lo[k]); b.hi[k] = fmaxf(b.hi[k], o.hi[k]); }
            b.nonfinite += o.nonfinite;
            n += s_live[w];
        }
        ExportTile &r = tiles[t];
#pragma unroll
        for (int k = 0; k < EXPORT_SUMS; k++) r.sum[k] = b.sum[k];
#pragma unroll
        for (int k = 0; k < 4; k++) { r.lo[k] = b.lo[k]; r.hi[k] = b.hi[k]; }
        r.nonfinite = b.nonfinite;
        tile_count[t] = n;
    }
}

// Workgroup 0 of pass B.  The fp64 sums take the tiles in index order, one sum to a thread (tile_order_sums: a serial
// chain, so the same bits on every run -- graphs or not -- for a given context geometry).  The extrema and counts do not
// depend on the order: every thread takes its tiles', then a tree.
__device__ __forceinline__ void export_finish(int ntiles, const int *__restrict__ tile_count, const ExportTile *__restrict__ tiles,
                                              int64_t *__restrict__ count_out, psamd_live_stats *__restrict__ stats_out)
{
    __shared__ float s_lo[SLOT_WAVES][4], s_hi[SLOT_WAVES][4];
    __shared__ int s_n[SLOT_WAVES][2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float lo[4], hi[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { lo[k] = __int_as_float(0x7f800000); hi[k] = -__int_as_float(0x7f800000); }
    int live = 0, nonfinite = 0;
    const double sum = tile_order_sums<EXPORT_SUMS>(ntiles, [&](int t, double (&v)[EXPORT_SUMS]) {
        const ExportTile r = tiles[t];
#pragma unroll
        for (int k = 0; k < EXPORT_SUMS; k++) v[k] = r.sum[k];
#pragma unroll
        for (int k = 0; k < 4; k++) { lo[k] = fminf(lo[k], r.lo[k]); hi[k] = fmaxf(hi[k], r.hi[k]); }
        nonfinite += r.nonfinite;
        live += tile_count[t];
    });
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; k++) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], m)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], m)); }
        live += __shfl_xor(live, m);
        nonfinite += __shfl_xor(nonfinite, m);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) { s_lo[wv][k] = lo[k]; s_hi[wv][k] = hi[k]; }
        s_n[wv][0] = live; s_n[wv][1] = nonfinite;
    }
    __syncthreads();
    psamd_live_stats *o = stats_out;
    switch (tid) {
    case 0: o->mass = sum; break;
    case 1: case 2: case 3: o->momentum[tid - 1] = sum; break;
    case 4: o->kinetic = sum; break;
    case 5: case 6: case 7: o->mass_moment[tid - 5] = sum; break;
    case 8: o->age_sum = sum; break;
    case 64: {
        long long n = 0, nf = 0;
        for (int w = 0; w < SLOT_WAVES; w++) {
            n += s_n[w][0]; nf += s_n[w][1];
#pragma unroll
            for (int k = 0; k < 4; k++) { lo[k] = fminf(lo[k], s_lo[w][k]); hi[k] = fmaxf(hi[k], s_hi[w][k]); }
        }
        for (int k = 0; k < 3; k++) { o->lo[k] = (double)lo[k]; o->hi[k] = (double)hi[k]; }
        o->age_min = (double)lo[3]; o->age_max = (double)hi[3];
        o->live = n; o->nonfinite = nf;
        *count_out = n;
        break;
    }
    default: break;
    }
}

// Pass B.  The same walk as pass A over tile blockIdx.x - 1.
__global__ __launch_bounds__(SLOT_THREADS) void k_export_write(DevParams P, int ntiles, const int *__restrict__ cell,
                                                               const float4 *__restrict__ pos4,
                                                               const float4 *__restrict__ vel4,
                                                               const float4 *__restrict__ acc4,
                                                               const int *__restrict__ tile_count,
                                                               const ExportTile *__restrict__ tiles, ExportFields out,
                                                               int64_t capacity, int64_t *__restrict__ count_out,
                                                               psamd_live_stats *__restrict__ stats_out)
{
    if (blockIdx.x == 0) { export_finish(ntiles, tile_count, tiles, count_out, stats_out); return; }
    if (!out.pos4 && !out.vel4 && !out.acc4 && !out.id && !out.cell) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, t = blockIdx.x - 1;
    const int before = tiles_before(tile_count, t);       // the live particles of the tiles before this one
    const int first = slot_first(t, wv, lane);
    unsigned long long mask[SLOT_ITEMS];
    int c[SLOT_ITEMS], live = 0;
#pragma unroll
    for (int k = 0; k < SLOT_ITEMS; k++) {
        c[k] = slot_cell(P, cell, first + 64 * k);
        mask[k] = __ballot(slot_live(P, c[k]));
        live += __popcll(mask[k]);
    }
    int64_t at = wave_offset<int64_t>(before, live, wv, lane);
    if (at >= capacity) return;                           // (the wave's slots all fall past the caller's capacity)
    // a batch's loads together, then its stores
#pragma unroll
    for (int k0 = 0; k0 < SLOT_ITEMS; k0 += EXPORT_BATCH) {
        float4 p[EXPORT_BATCH], v[EXPORT_BATCH], a[EXPORT_BATCH];
        int64_t o[EXPORT_BATCH];
#pragma unroll
        for (int k = 0; k < EXPORT_BATCH; k++) {
            const unsigned long long m = mask[k0 + k];
            o[k] = at + (int64_t)lane_rank(m);
            at += __popcll(m);
            if (((m >> lane) & 1ull) && o[k] < capacity) {
                const int i = first + 64 * (k0 + k);
                if (out.pos4) p[k] = pos4[i];
                if (out.vel4) v[k] = vel4[i];
                if (out.acc4) a[k] = acc4[i];
            }
        }
#pragma unroll
        for (int k = 0; k < EXPORT_BATCH; k++) {
            if (((mask[k0 + k] >> lane) & 1ull) && o[k] < capacity) {
                const int i = first + 64 * (k0 + k);
                if (out.pos4) out.pos4[o[k]] = p[k];
                if (out.vel4) out.vel4[o[k]] = v[k];
                if (out.acc4) out.acc4[o[k]] = a[k];
                if (out.id) out.id[o[k]] = slot_of_index(P, i);
                if (out.cell) out.cell[o[k]] = c[k0 + k];
            }
        }
    }
}

hipError_t launch_export_live(hipStream_t st, const DevParams &P, const DeviceState &d, const ExportFields &out,
                              int64_t capacity, int64_t *count_out, psamd_live_stats *stats_out)
{
    const int ntiles = slot_tiles(P.slots_total);
    if (ntiles > 0) {
        k_export_count<<<ntiles, SLOT_THREADS, 0, st>>>(P, d.cell, d.pos4, d.vel4, d.exp_count, d.exp_tiles);
        PS_LAUNCH_CHECK();
    }
    k_export_write<<<ntiles + 1, SLOT_THREADS, 0, st>>>(P, ntiles, d.cell, d.pos4, d.vel4, d.acc4, d.exp_count, d.exp_tiles,
                                                          out, capacity, count_out, stats_out);
    PS_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace psamd
