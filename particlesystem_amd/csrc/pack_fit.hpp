// pack_fit.hpp -- which partly filled last slices share a wave: the rule, written once, serially
//
// The two-pass force pass walks a cell's full 64-slices as ordinary tasks; a cell's leftover r = active_count & 63
// (r > 0) rides in a pack, a wave that carries up to PACK_GROUPS cells' leftovers side by side in its PACK_LANES lanes
// (merged_pack_task).  A pack's walk costs about the same whatever its fill, so the rule is to need few packs:
//   * the computed cells, in comp_cell order, in windows of PACK_WINDOW consecutive cells;
//   * inside a window the leftovers by decreasing r, ties in cell order;
//   * each goes into the open pack of its window that it leaves the least room in (open: fewer than PACK_GROUPS cells and
//     used + r <= PACK_LANES), ties to the lowest pack number; none fits: a new pack;
//   * packs are numbered window by window, inside a window in the order they were opened; a pack lists its cells in
//     the order they were placed.
// (Best fit decreasing.  On 4096 cells of Poisson(256) bodies, 57.9 % of them active, it needs 0.76 times the packs of
// the next fit over runs of six cells it replaced, lane fill 94 % against 72 %.)
// A pure function of the leftovers.  plan.hip's k_pack_windows is the same rule with a wave per window, the lanes standing
// for the packs.  tests/pack_fit_model.py restates the rule in Python: tests/test_pack_fit_cpu.py compares this text with it
// pack for pack, tests/test_gpu_pack_fit.py the device's packs (psamd_debug_packs).
// Host and device inline code, no HIP types.
#pragma once

#if defined(__HIPCC__)
#define PACK_FIT_HD __host__ __device__
#else
#define PACK_FIT_HD
#endif

namespace psamd {

constexpr int PACK_WINDOW = 64;     // cells per window (a power of two: a wave's lanes hold a window)
constexpr int PACK_LANES = 64;      // lanes of a pack
constexpr int PACK_GROUPS = 4;      // cells of a pack at most (merged_pack_task's LDS tiles)

// One window: the leftovers r[0 .. n), n <= PACK_WINDOW, each in 0 .. PACK_LANES - 1.  out (may be null): PACK_GROUPS ints
// per pack, base + index into r, -1 for an unused place.  Returns the number of packs.
PACK_FIT_HD inline int pack_fit_window(const int *r, int n, int base, int *out)
{
    int order[PACK_WINDOW], m = 0;
    for (int i = 0; i < n; i++) {                // decreasing r, ties in cell order (a stable insertion)
        if (r[i] <= 0) continue;
        int k = m++;
        while (k > 0 && r[order[k - 1]] < r[i]) { order[k] = order[k - 1]; k--; }
        order[k] = i;
    }
    int used[PACK_WINDOW], ng[PACK_WINDOW], np = 0;
    for (int k = 0; k < m; k++) {
        const int i = order[k];
        int best = -1;
        for (int b = 0; b < np; b++)
            if (ng[b] < PACK_GROUPS && used[b] + r[i] <= PACK_LANES && (best < 0 || used[b] > used[best])) best = b;
        if (best < 0) {
            best = np++;
            used[best] = 0; ng[best] = 0;
            if (out) for (int s = 0; s < PACK_GROUPS; s++) out[PACK_GROUPS * best + s] = -1;
        }
        if (out) out[PACK_GROUPS * best + ng[best]] = base + i;
        used[best] += r[i];
        ng[best]++;
    }
    return np;
}

// All windows of the leftovers r[0 .. n).  out (may be null: the count pass) as above, indices into r.
PACK_FIT_HD inline int pack_fit(const int *r, int n, int *out)
{
    int np = 0;
    for (int w0 = 0; w0 < n; w0 += PACK_WINDOW)
        np += pack_fit_window(r + w0, n - w0 < PACK_WINDOW ? n - w0 : PACK_WINDOW, w0, out ? out + PACK_GROUPS * np : nullptr);
    return np;
}

}  // namespace psamd
