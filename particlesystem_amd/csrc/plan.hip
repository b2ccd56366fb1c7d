// plan.hip -- the plan of the balanced force pass: task list, packs, where every wave slot starts
#include "balanced.hpp"
#include "pack_fit.hpp"

namespace psamd {

// The largest of a wave's values (any ints), as a wave-uniform number: the row scan and the two
// row broadcasts of the DPP network, the whole wave active.
__device__ __forceinline__ int wave_max(int v)
{
#define PS_MAX_STEP(ctrl, rows) v = max(v, __builtin_amdgcn_update_dpp(v, v, ctrl, rows, 0xf, false))
    PS_MAX_STEP(0x111, 0xf);      // row_shr:1, 2, 4, 8: lane 15 of every row of 16 holds its row's largest
    PS_MAX_STEP(0x112, 0xf);
    PS_MAX_STEP(0x114, 0xf);
    PS_MAX_STEP(0x118, 0xf);
    PS_MAX_STEP(0x142, 0xa);      // row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3: lane 63 holds the wave's
    PS_MAX_STEP(0x143, 0xc);
#undef PS_MAX_STEP
    return __builtin_amdgcn_readlane(v, 63);
}

// The packs of the leftovers (pack_fit.hpp holds the rule and its reasons), a wave per window of PACK_WINDOW computed cells,
// ahead of k_plan_force: best fit is a chain of dependent placements, about 55 instructions each (counted in the ISA), and 64
// windows of up to 63 placements are by that count more than the plan's one workgroup could issue beside its own work;
// side by side on CUs of their own a window is one chain: the kernel takes 13 us (profiles/pack_fit_ab.txt).  The lanes first hold the window's cells
// (rank by decreasing leftover: 64 compares of distinct keys), then the sorted leftovers move to the lanes of their rank and
// the lanes stand for the packs: a placement is one compare per pack, one wave_max over (used, lowest pack number first)
// and the update of the pack that won.  Leftovers above half a wave cannot share one with anything placed before them:
// they open packs rank by rank without the loop.  The window's packs go to pack_stage[64 w ..], their number to
// pack_count[w]; k_plan_force numbers the windows' packs and moves them into merged_tasks.
__global__ __launch_bounds__(PACK_WINDOW) void k_pack_windows(DevParams P, const int *__restrict__ active_count,
                                                              int4 *__restrict__ pack_stage, int *__restrict__ pack_count)
{
    static_assert(PACK_WINDOW == 64 && PACK_LANES == 64 && PACK_GROUPS == 4, "a wave's lanes hold a window; a pack is an int4");
    const int lane = threadIdx.x, w = blockIdx.x, j = w * PACK_WINDOW + lane;
    const int cell = j < comp_count(P) ? comp_cell(P, j) : -1;
    const int r = cell >= 0 ? (active_count[cell] & (PACK_LANES - 1)) : 0;
    const int key = (r << 6) | (63 - lane);                  // decreasing leftover, ties in cell order
    int rank = 0;
#pragma unroll
    for (int i = 0; i < 64; i++) rank += __builtin_amdgcn_readlane(key, i) > key ? 1 : 0;
    const int sr = __builtin_amdgcn_ds_permute(rank << 2, r);          // lane k: the k-th leftover in that order, and its cell
    const int sc = __builtin_amdgcn_ds_permute(rank << 2, cell);
    const int nitems = __popcll(__ballot(r > 0)), nbig = __popcll(__ballot(r > PACK_LANES / 2));
    constexpr int CLOSED = 1 << 20;                          // a pack not open yet, or with its four cells: nothing fits
    int used = lane < nbig ? sr : CLOSED, ng = lane < nbig ? 1 : 0;    // lane b as pack b
    int mypack = lane, myplace = 0;                          // lane k as the k-th leftover: where it went
    int nopen = nbig;
    for (int k = nbig; k < nitems; k++) {
        const int rk = __builtin_amdgcn_readlane(sr, k);
        const int best = wave_max(used <= PACK_LANES - rk ? ((used << 6) | (63 - lane)) : -1);
        int b, nu, ngb = 0;
        if (best < 0) { b = nopen++; nu = rk; }
        else { b = 63 - (best & 63); nu = (best >> 6) + rk; ngb = __builtin_amdgcn_readlane(ng, b); }
        if (ngb == PACK_GROUPS - 1) nu = CLOSED;
        if (lane == b) { used = nu; ng = ngb + 1; }
        if (lane == k) { mypack = b; myplace = ngb; }
    }
    int *out = reinterpret_cast<int *>(pack_stage + (size_t)w * PACK_WINDOW);
    if (lane < nitems) out[PACK_GROUPS * mypack + myplace] = sc;
    if (lane < nopen) for (int s = ng; s < PACK_GROUPS; s++) out[PACK_GROUPS * lane + s] = -1;
    if (lane == 0) pack_count[w] = nopen;
}

// The plan of the balanced force pass, one launch of eight workgroups (one per XCD run of wave
// slots).  Every workgroup works out, for itself, in LDS:
//   (1) the prefix over the computed cells (the lent ones first: their results travel back to the
//       rank that owns them) of the 64-slices of the active lists and of what those tasks walk
//       (a task of cell c walks task_cost[c] bodies, the population of the cell's stencil);
//       with `merge`, only full slices become ordinary tasks and the leftovers (a cell's last,
//       partly filled slice: 20 of 64 lanes on average once the collided particles are gone) are
//       packed, up to four cells to a wave, into merged tasks (k_pack_windows, just before this kernel);
//   (2) where every wave slot of ITS run starts: the pass's work is the list of (task, stencil
//       step) units -- task-major, 27 steps per task -- a unit costs the bodies of the neighbour
//       cell it visits, and wave slot s takes the units from wave_pos[s] up to wave_pos[s + 1]:
//       equal shares of the cost, cut at unit boundaries.  The eight runs start at whole tasks, so a
//       task that is cut is always continued by a workgroup of the same run.
// The task list, the packs and the frame scalars are the same whichever workgroup writes them; each
// writes a share.  (These were three launches, k_build_active / k_active_tasks / k_split_tasks, 60 us
// of mostly one-workgroup latency on the step's critical path; the prefixes are cheap enough to
// be recomputed eight times.)
// merge: false every slice is an ordinary task; true the packs are walked by the first workgroups of the
// balanced pass (merged_pack_task), beside its ordinary tasks.
constexpr int PLAN_LDS = 6144;        // prefix entries (computed cells + 1) kept in LDS
__global__ __launch_bounds__(1024) void k_plan_force(DevParams P, int nw, bool merge, const int *__restrict__ cell_start_g,
                                                     const int *__restrict__ active_count, const int *__restrict__ task_cost,
                                                     int *__restrict__ task_list2, int *__restrict__ ctask_start_g,
                                                     long long *__restrict__ cost_start_g, int4 *__restrict__ merged_tasks,
                                                     const int4 *__restrict__ pack_stage, const int *__restrict__ pack_count, int *__restrict__ pack_base_g,
                                                     long long *__restrict__ wave_pos, FrameScalars *fs, unsigned long long *trace,
                                                     StepState *st, int pass)
{
#ifdef PSAMD_PLAN_TRACE    // diagnostic build: time stamps (100 MHz) of workgroup x's phases in trace[8 x ...]
#define PT(i) do { if (threadIdx.x == 0) trace[8 * blockIdx.x + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define PT(i) do {} while (0)
#endif
    PT(0);
    __shared__ long long s_cost[PLAN_LDS + 1];
    __shared__ int s_task[PLAN_LDS + 1];
    __shared__ int s_ac[PLAN_LDS];                     // active_count | task_cost << 13 of the j-th computed cell
    __shared__ long long wave_tot[16], wave_cost[16];
    __shared__ long long s_run[2];
    __shared__ long long s_runcost[2];
    __shared__ int s_pbase[PLAN_LDS / PACK_WINDOW + 1];  // first pack of every window
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, x = blockIdx.x;
    const int ncomp = comp_count(P);
    const bool in_lds = ncomp + 1 <= PLAN_LDS && P.max_per_cell < (1 << 13);
    long long *cost_start = in_lds ? s_cost : cost_start_g;
    int *ctask_start = in_lds ? s_task : ctask_start_g;
    int *pack_base = in_lds ? s_pbase : pack_base_g;
    if (in_lds) for (int j = tid; j < ncomp; j += 1024) { const int c = comp_cell(P, j), n = active_count[c]; s_ac[j] = n | ((n ? task_cost[c] : 0) << 13); }
    __syncthreads();
    PT(1);
    auto act_of = [&](int j) { return in_lds ? (s_ac[j] & 0x1fff) : active_count[comp_cell(P, j)]; };
    auto cost_of = [&](int j) { return in_lds ? (s_ac[j] >> 13) : task_cost[comp_cell(P, j)]; };

    // ---- (1) prefixes, task list, packs ----
    const int per = (ncomp + 1023) / 1024;
    const int c0 = min(ncomp, tid * per), c1 = min(ncomp, c0 + per);
    // the packs of the leftovers: k_pack_windows listed every window's packs and counted them; here they are numbered,
    // window by window (the counts ride in the high word of the tasks' prefix), and workgroup 0 moves them into place
    const int nwin = (ncomp + PACK_WINDOW - 1) / PACK_WINDOW, wper = (nwin + 1023) / 1024;
    const int w0 = min(nwin, tid * wper), w1 = min(nwin, w0 + wper);
    long long mine = 0, mycost = 0;   // tasks (low word) and packs (high word); bodies the tasks walk
    for (int j = c0; j < c1; j++) {
        const int n = act_of(j), nt = merge ? (n >> 6) : ((n + 63) >> 6);
        mine += nt;
        mycost += (long long)nt * cost_of(j);
    }
    if (merge) {
        int np = 0;
        for (int w = w0; w < w1; w++) np += pack_count[w];
        mine |= (long long)np << 32;
    }
    long long incl = mine, cincl = mycost;
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(incl, d), oc = __shfl_up(cincl, d);
        if (lane >= d) { incl += o; cincl += oc; }
    }
    if (lane == 63) { wave_tot[wv] = incl; wave_cost[wv] = cincl; }
    __syncthreads();
    long long run2 = incl - mine, total2 = 0, crun = cincl - mycost, ctotal = 0;
    for (int k = 0; k < 16; k++) {
        if (k < wv) { run2 += wave_tot[k]; crun += wave_cost[k]; }
        total2 += wave_tot[k]; ctotal += wave_cost[k];
    }
    int run = (int)(run2 & 0xffffffffll);
    const int total = (int)(total2 & 0xffffffffll), npacks = (int)(total2 >> 32);
    PT(2);
    const bool my_share = (tid & 7) == x;           // the lists in memory: each workgroup writes an eighth
    for (int j = c0; j < c1; j++) {
        const int n = merge ? (act_of(j) >> 6) : ((act_of(j) + 63) >> 6);
        ctask_start[j] = run; cost_start[j] = crun;
        if (my_share && n) { const int c = comp_cell(P, j); for (int sl = 0; sl < n; sl++) task_list2[run + sl] = c * P.slices + sl; }
        run += n;
        crun += (long long)n * cost_of(j);
    }
    if (merge && x == 0) {
        int first = (int)(run2 >> 32);
        for (int w = w0; w < w1; w++) { pack_base[w] = first; first += pack_count[w]; }
    }
    const int ntask = total;
    const long long T = ctotal;
    if (tid == 0) {
        ctask_start[ncomp] = ntask;
        cost_start[ncomp] = T;
        if (x == 0) { fs->n_tasks2 = total; fs->n_merged = npacks; fs->cost_total = T; }
    }
    if (!in_lds) __threadfence();                    // (every workgroup wrote the same values; this one reads its own)
    __syncthreads();
    PT(3);
    if (merge && x == 0)
        for (int i = tid; i < nwin * PACK_WINDOW; i += 1024) {
            const int w = i / PACK_WINDOW, l = i - w * PACK_WINDOW;
            if (l < pack_count[w]) merged_tasks[pack_base[w] + l] = pack_stage[i];
        }
    if (nw <= 0) return;                             // (unbalanced pass: only the lists were wanted)

    // ---- (2) the wave slots of run x ----
    // A position in the pass's work is (task, cost already walked inside the task): which stencil step
    // that is depends on the populations of the task's stencil, which the wave that starts (or stops)
    // there looks up anyway -- k_pairs_balanced turns the residual into a step.  (Walking the 27 counts
    // here, per wave slot, was most of this kernel's 40 us.)  whole = round up to the next task start.
    auto pos_at = [&](long long v, bool whole) -> long long {
        if (v >= T) return wave_pos_make(ntask, 0);
        int a = 0, b = ncomp - 1;                         // last cell whose tasks start at or before v
        while (a < b) { const int m = (a + b + 1) >> 1; if (cost_start[m] <= v) a = m; else b = m - 1; }
        const int nt = ctask_start[a + 1] - ctask_start[a];
        const int S = cost_of(a);
        if (nt == 0 || S <= 0) return wave_pos_make(ctask_start[a + 1], 0);     // (v < T: cannot be the last cell)
        const long long off = v - cost_start[a];
        const int q = (int)min((long long)(nt - 1), off / S);
        const int r = (int)(off - (long long)q * S);
        const int t = ctask_start[a] + q;
        if (whole) return wave_pos_make(t + (r > 0 ? 1 : 0), 0);
        return wave_pos_make(t, r);
    };
    auto cost_of_task_start = [&](int t) -> long long {
        if (t >= ntask) return T;
        int a = 0, b = ncomp - 1;
        while (a < b) { const int mm = (a + b + 1) >> 1; if (ctask_start[mm] <= t) a = mm; else b = mm - 1; }
        return cost_start[a] + (long long)(t - ctask_start[a]) * cost_of(a);
    };
    const int m = nw >> 3;                                // wave slots per XCD run (nw is a multiple of 32)
    if (tid < 2) {
        s_run[tid] = pos_at(T * (x + tid) / 8, true);
        s_runcost[tid] = cost_of_task_start(wave_pos_task(s_run[tid]));
    }
    __syncthreads();
    PT(4);
    const long long run_lo = s_run[0], run_hi = s_run[1];
    const long long lo = s_runcost[0], hi = s_runcost[1];
    for (int j = tid; j < m; j += 1024)                   // equal shares of the run's own cost range
        wave_pos[x * m + j] = j == 0 ? run_lo : max(run_lo, min(run_hi, pos_at(lo + (hi - lo) * j / m, false)));
    if (x == 7 && tid == 0) wave_pos[nw] = run_hi;        // = (ntask, 0)
    if (x == 0 && tid == 0) {
        // the clock of the pass that follows (WavePace): how long the last one took, and when this one was planned
        const unsigned long long a = st->pairs_t0[pass], b = st->pairs_end[pass];
        st->pairs_ticks[pass] = (b > a && b - a < (1ull << 30)) ? (int)(b - a) : 0;
        st->pairs_t0[pass] = __builtin_amdgcn_s_memrealtime();
        st->pairs_end[pass] = 0;
    }
    __syncthreads();
    PT(5);
#undef PT
}

// nw: wave slots of the balanced pass (0: only the lists are wanted); merge: pack the partly filled last slices
void launch_plan_force(hipStream_t st, const DevParams &P, const DeviceState &d, int nw, bool merge, int pass)
{
    if (merge) k_pack_windows<<<(comp_count(P) + PACK_WINDOW - 1) / PACK_WINDOW, PACK_WINDOW, 0, st>>>(P, d.active_count, d.pack_stage, d.pack_count);
    k_plan_force<<<8, 1024, 0, st>>>(P, nw, merge, d.cell_start, d.active_count, d.task_cost,
                                     d.task_list2, d.ctask_start, d.cost_start, d.merged_tasks, d.pack_stage, d.pack_count, d.pack_base, d.wave_pos, d.fs, d.trace, d.st, pass);
}

}  // namespace psamd
