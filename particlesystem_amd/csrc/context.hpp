// context.hpp -- the psamd context and what the host units share (create.hip, step.hip, io.hip, services.hip).
//
// Host side of the drop-in boundary, C++ like the reference's host code.  It mirrors
// the reference driver's view of the path: nine buffers (ps.cpp:70-78), one-off setup
// stages, then per step init_iframe -> build_grid -> calc_forces (ps.cpp:1843-1928).
// All arithmetic of the step runs in the HIP kernels (kernels_common.hpp holds the map); there
// is no CPU fallback: without a HIP device psamd_create fails with PSAMD_ERR_NO_DEVICE.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/psamd.h"
#include "context_params.hpp"
#include "device_types.h"
#include "frame_stage.hpp"
#include "geometry.hpp"
#include "kernels.h"
#include "partition.hpp"
#include "step_ledger.hpp"

namespace psamd {
// a slab message's buffer (device), by the MSG_* numbering of context_params.hpp
struct SlabMsg {
    int *ptr = nullptr;
    size_t bytes = 0, alloc = 0;    // what travels now; the buffer's room (they differ for MSG_XFER_*: bytes grows with P.xfer_cap)
};
// the kinds of stage sequence that are captured as hipGraphs (step.hip: run_segment)
enum { SEG_BUILD = 0, SEG_PAIRS, SEG_APPLY, SEG_FINISH, SEG_STEP, NSEG };
}  // namespace psamd

using namespace psamd;      // (a private header: every host unit speaks these types)

struct psamd_ctx {
    Geometry geo;
    DevParams P{};
    DevParams P_int{}, P_rest{};      // the pair stage cut in two: interior own cells (no halo needed), the rest
    bool have_interior = false;
    SegLayout S{};
    DeviceState d;
    hipStream_t stream = nullptr;       // stream in use
    hipStream_t own_stream = nullptr;   // the one this context created
    SlabPlan plan;
    SlabMsg msg[MSG_COUNT];
    int halo_out_c0[2] = {0, 0}, halo_out_cells[2] = {0, 0}, halo_in_cells[2] = {0, 0};
    int *pack_off[2] = {nullptr, nullptr}, *unpack_off[2] = {nullptr, nullptr};
    size_t frame_ints = 0;            // ints zeroed by init_iframe
    std::vector<void *> allocs;
    std::string err;
    // host mirrors
    std::vector<CellInfo> celltab;
    std::vector<QueueInfo> h_qinfo;   // with h_queue the host's mirror of the queues, current while host_queues_valid
    std::vector<int32_t> h_queue;
    bool host_queues_valid = true;    // host mirror == device copy
    FrameScalars *h_fs = nullptr;     // pinned host copies of the per-frame scalars: TWO records, a step's number picks one
    StepLedger ledger;                // the steps enqueued, their records read and what follows from them (step_ledger.hpp)
    char *snapshot = nullptr;         // device image for snapshot_save / _restore
    int snapshot_step = 0;
    void *staging = nullptr;          // device staging for AoS transfers
    size_t staging_bytes = 0;
    Stage stage = ST_IDLE;            // where the host stands in the frame in progress: moved by enter / leave alone (frame_stage.hpp)
    bool tdata_mirror = true;         // build_grid also writes the reference's T_DATA rows (psamd_set_tdata_mirror)
    bool frame_clean = true;          // the per-frame counts are zero: a finished step leaves them so (its last kernel is the next init_iframe)
    int step = 0;
    int64_t steps_total = 0;
    uint64_t pairs_shape_last = 0;    // launch_pairs_shape of the last pair-stage launch (psamd_debug_packs)
    InjectScratch inj{};              // its scratch: inj.e grows with max_count, the rest is fixed
    RemoveScratch rem{};              // psamd_remove's scratch: rem.e grows with max_count, the rest is fixed
    ProbeScratch prb{};               // psamd_probe's scratch: code / order grow with max_count, the counters are fixed
    UpdateScratch upd{};              // psamd_update's scratch: code grows with max_count, the rest is fixed (by id it borrows rem.claim)
    DepositScratch dep{};             // psamd_deposit's scratch: fixed (the geometry and the plan size it)
    SampleScratch smp{};              // psamd_sample's scratch: fixed (three counters; by export order it borrows upd.tile_live)
    NbrScratch nbr{};                 // psamd_neighbours' scratch: one block the first call allocates, sized by the container alone
    GrpScratch grp{};                 // psamd_groups' scratch: one block the first call allocates, sized by the container alone
    KnnScratch knn{};                 // psamd_knn's scratch: one block the first call allocates, sized by the container alone (not by k)
    // timing
    int timing = 0;                   // 0 off, 1 pair pass / apply / life cycle, 2 every stage
    int timing_period = 1;             // events are recorded on every timing_period-th step since set_timing
    int64_t timing_steps = 0;          // steps since set_timing
    int timing_now = 0;                // the level in force for the step being run (0 on the steps in between)
    bool wedged = false;               // a step's scalars did not arrive within the wall-clock bound: the context refuses further work
    // Timing events: two sets, a timed step takes the one that was read longest ago; a set is read when it is taken again
    // or by psamd_get_timing -- never by the step that recorded it (the host runs ahead of the GPU).
    enum { E_RESET = 0, E_HIST, E_SCAN, E_SCATTER, E_SORT, E_SORT_END, E_COLLIDE, E_FORCE, E_PAIRS_END, E_APPLY, E_LIFE, E_END, E_COUNT };
    hipEvent_t ev[2][E_COUNT]{};
    int ev_level[2] = {0, 0};          // level a set was recorded at, 0: nothing outstanding in it
    int tset = 0;                      // the set of the step being run
    int64_t timed_steps = 0;
    bool ev_made = false;
    double t_us[PSAMD_NUM_TIMERS]{};
    std::vector<float> t_samples[PSAMD_NUM_TIMERS];
    int64_t t_launches = 0;
    // stage sequences as hipGraphs (psamd_set_graphs): per kind of sequence, the shapes captured so far
    struct GraphSlot { uint64_t key; hipGraphExec_t exec; uint64_t stamp; };
    bool graphs = false;
    std::vector<GraphSlot> gcache[NSEG];
    uint64_t gstamp = 0;
    int64_t graph_launches = 0, graph_captures = 0;
    std::string graph_refused;         // why the runtime would not capture (the context then runs without graphs)
    int64_t slab_bound = 0;            // the bound slab_apply sized its launches from; slab_finish uses the same
    int wait_policy = 0;               // how the host waits for the step's scalars: 0 spin, 1 spin briefly, then nap
    double wait_limit_s = 10.0;        // ... and for how long at most (PSAMD_WAIT_LIMIT_S)
};

namespace psamd {

const char *status_text(int status);

// what the ledger's rules read of the context
inline LedgerParams ledger_params(const psamd_ctx *c)
{
    const DevParams &P = c->P;
    return {P.slots_total, (P.flags & PSAMD_FLAG_EXPLOSIONS) != 0, P.world, P.xfer_cap, P.xfer2_cap, P.far_cap, P.xfer_cap0, P.xfer_cap_max,
            comp_count(P), comp_count(c->P_int), comp_count(c->P_rest), P.world > 1 ? (int64_t)P.world * STATUS_KILL_CAP : 0, BUCKET_MAX};
}

inline int fail(psamd_ctx *c, int status, const std::string &what)
{
    if (c) c->err = std::string(status_text(status)) + ": " + what;
    return status;
}

inline int hip_fail(psamd_ctx *c, hipError_t e, const char *what)
{
    return fail(c, e == hipErrorOutOfMemory ? PSAMD_ERR_OUT_OF_MEMORY : PSAMD_ERR_HIP,
                std::string(what) + ": " + hipGetErrorString(e));
}

#define PS_HIP(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hip_fail((c), e_, #call); } while (0)
#define PS_TRY(call) do { const int rc_ = (call); if (rc_ != PSAMD_OK) return rc_; } while (0)     // a status passed up

template <typename T>
hipError_t dev_alloc(psamd_ctx *c, T **out, size_t n)
{
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) return e;
    c->allocs.push_back(p);
    *out = (T *)p;
    // PSAMD_POISON (tests): fresh device memory is usually zero, reused memory is not -- fill every
    // allocation with a pattern so that anything read before it is written shows up
    static const bool poison = std::getenv("PSAMD_POISON") != nullptr;
    if (poison) {
        e = hipMemset(p, 0xA5, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) e = hipDeviceSynchronize();     // (the fill must not overtake the context's own stream)
    }
    return e;
}

// internals that cross the host units
int pull_queues(psamd_ctx *c);                      // io.hip: device -> host mirror
int push_queues(psamd_ctx *c);                      // ... host mirror -> device
int check_device_errors(psamd_ctx *c);              // step.hip: after a sync, the sticky error bits raised by kernels
int drain_scalars(psamd_ctx *c, bool quiet = false);
int refuse_wedged(psamd_ctx *c);
int ensure_staging(psamd_ctx *c, size_t bytes);     // io.hip: the device staging buffer holds at least so many bytes
void end_frame(psamd_ctx *c, Call why = CALL_CHANGED);  // services.hip: the slots or queues changed under the host's frame
void drop_graphs(psamd_ctx *c);

}  // namespace psamd
