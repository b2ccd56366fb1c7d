// step.hip -- the stage engine: timing events, the enq_* stages, the hipGraph cache, the scalar-record pipeline, the
// one-GPU stage calls, psamd_step, the slab stages, psamd_synchronize and the setters that steer them.
#include <atomic>
#include <ctime>

#include <sys/prctl.h>

#include "context.hpp"

int psamd::check_device_errors(psamd_ctx *c)
{
    FrameScalars fs{};
    PS_HIP(c, hipMemcpy(&fs, c->d.fs, sizeof fs, hipMemcpyDeviceToHost));
    if (!built(c->stage)) for (int k = 0; k < 5; k++) fs.n_out[k] = c->ledger.last().n_out[k];      // (between steps the device's record is the next frame's, zeroed)
    if (fs.error & (ERR_BAD_ID | ERR_BAD_POS)) {
        // an upload error is reported once and then cleared: the rejected records stay in the
        // container, the caller is expected to upload valid ones over them
        const int bits = fs.error;
        const int cleared = fs.error & ~(ERR_BAD_ID | ERR_BAD_POS);
        (void)hipMemcpy(&c->d.fs->error, &cleared, sizeof(int), hipMemcpyHostToDevice);
        return fail(c, PSAMD_ERR_INVALID_ARG, (bits & ERR_BAD_ID) ? "uploaded particle with id != slot index"
                                                                  : "uploaded live particle outside the box or with cell >= NUM_CELLS");
    }
    if (fs.error & ERR_CELL_TOO_BIG) return fail(c, PSAMD_ERR_CELL_OVERFLOW, "a cell holds more particles than the sort kernel ranks");
    if (fs.error & ERR_FOREIGN_CELL) return fail(c, PSAMD_ERR_STATE, "a particle stored on this rank sits in a cell layer the rank holds no state for");
    if (fs.error & ERR_HALO_OVERFLOW) {
        // say what was asked for, so that the caller can size the messages (the error may also have come in with a
        // neighbour's message header: then the numbers below are this rank's own and may all fit)
        char buf[512];
        std::snprintf(buf, sizeof buf, "a slab message had no room (raise halo_cap_cell / xfer_cap): this step this rank wanted to send %d / %d "
                      "transfer records down / up (room: %d each now -- it follows the traffic two steps behind, up to xfer_cap_max), %d / %d two ranks away (room %d), %d to a far rank (room %d); "
                      "a halo message holds halo_cap_cell = %d bodies per cell on average over a cell layer",
                      fs.n_out[0], fs.n_out[1], c->P.xfer_cap, fs.n_out[2], fs.n_out[3], c->P.xfer2_cap, fs.n_out[4], c->P.far_cap, c->P.halo_cap_cell);
        return fail(c, PSAMD_ERR_CELL_OVERFLOW, buf);
    }
    if (fs.error & ERR_SLAB_MISMATCH) return fail(c, PSAMD_ERR_STATE, "a slab message does not match the receiver's plan or counts");
    if (fs.error & ERR_REMOTE_RECORD0) return fail(c, PSAMD_ERR_CELL_OVERFLOW, "more cell-overflow kills in one step than a slab's status message carries (ps.cpp:1523-1526 frees them into queue record 0)");
    if (fs.error & ERR_CHUNK_CAP) return fail(c, PSAMD_ERR_CELL_OVERFLOW, "a chunk list passed MAX_PARTICLES_PER_CHUNK: the reference skips its tail (ps.cpp:1502-1508), this library does not reproduce that");
    if (fs.error & ERR_OPS_OVERFLOW) return fail(c, PSAMD_ERR_CELL_OVERFLOW, "lifecycle op buffer overflow");
    if (fs.error & ERR_HANDOFF_TIMEOUT) return fail(c, PSAMD_ERR_STATE, "force pass: a wave never saw the partial sums of the task it continues");
    if (fs.error) return fail(c, PSAMD_ERR_STATE, "device error bits " + std::to_string(fs.error));
    return PSAMD_OK;
}

static void make_events(psamd_ctx *c)
{
    if (c->ev_made) return;
    for (auto &set : c->ev) for (auto &e : set) (void)hipEventCreate(&e);
    c->ev_made = true;
}

// read a set of timing events (waits for its step's last kernel: a set is read when it is taken again, two timed
// steps later, or by psamd_get_timing)
static void collect_timing(psamd_ctx *c, int set)
{
    const int level = c->ev_level[set];
    if (!level) return;
    c->ev_level[set] = 0;
    if (hipEventSynchronize(c->ev[set][psamd_ctx::E_END]) != hipSuccess) return;
    // timers: hist scan scatter sort | force pass, apply, life cycle | frame reset | flags + active lists (two-pass prologue)
    using X = psamd_ctx;
    const int a[PSAMD_NUM_TIMERS] = {X::E_HIST, X::E_SCAN, X::E_SCATTER, X::E_SORT, X::E_FORCE, X::E_APPLY, X::E_LIFE, X::E_RESET, X::E_COLLIDE};
    const int b[PSAMD_NUM_TIMERS] = {X::E_SCAN, X::E_SCATTER, X::E_SORT, X::E_SORT_END, X::E_PAIRS_END, X::E_LIFE, X::E_END, X::E_HIST, X::E_FORCE};
    for (int k = 0; k < PSAMD_NUM_TIMERS; k++) {
        if (level < 2 && (k < 4 || k == 7)) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev[set][a[k]], c->ev[set][b[k]]) == hipSuccess) {
            c->t_us[k] += 1000.0 * ms;
            c->t_samples[k].push_back(1000.0f * ms);
        }
    }
    c->t_launches++;
}

static void tick(psamd_ctx *c, int e)        // a timing event on the context's stream, if this step carries them
{
    if (c->timing_now) (void)hipEventRecord(c->ev[c->tset][e], c->stream);
}

// ---- stages ---------------------------------------------------------------------
//
// Every stage is a fixed sequence of kernel launches whose arguments do not change from step to step
// (sizes live on the device; the step's number and the scalar records' sequence number too: StepState).
// enq_* functions only enqueue; the host-side state machine is advanced by their callers -- so that a
// sequence can be captured once into a hipGraph and replayed (psamd_set_graphs): one submission per stage
// instead of one per kernel.  A graph is keyed by what shapes its launches: the size of the balanced force
// pass (from the last task count the host has seen) and the hint of the live count the life-cycle grids are sized
// from, rounded up to 64 Ki so that a free-running population does not mean a capture per step.  Steps
// that carry timing events run eagerly (the events sit between the kernels).
//
// Nothing in a step waits for the host; step_ledger.hpp has the pipeline of the scalar records, the hints and the verdicts.

static int slab_only(psamd_ctx *c, const char *what)
{
    return fail(c, PSAMD_ERR_STATE, std::string(what) + ": this context is one slab of a multi-rank system; step it with psamd_slab_build / "
                                                         "_pairs / _apply / _finish and exchange the messages in between");
}

int psamd::refuse_wedged(psamd_ctx *c)
{
    return fail(c, PSAMD_ERR_STATE, "the GPU stopped answering (a step's scalars did not arrive within " + std::to_string((int)c->wait_limit_s) +
                                    " s while its stream stayed busy): this context takes no further work; destroy it");
}

// The front of every stage call: a context, one that still answers, a call of the family a slab of several is stepped by,
// and the order test (frame_stage.hpp).  A refused call has touched nothing.
static int enter_stage(psamd_ctx *c, Call k)
{
    static const char *const plain[] = {"init_iframe", "build_grid", "calc_forces", "calc_forces", "step"};
    if (!c) return PSAMD_ERR_INVALID_ARG;
    if (c->wedged) return refuse_wedged(c);
    if (k < CALL_SLAB_BUILD && c->P.world > 1) return slab_only(c, plain[k]);
    const char *why = enter(c->stage, k);
    return why ? fail(c, PSAMD_ERR_STATE, why) : (int)PSAMD_OK;
}

// which steps carry timing events is settled when the step begins (before anything is enqueued or replayed)
static void begin_step(psamd_ctx *c)
{
    // (an event between two kernels costs ~6 us of idle GPU: a long timed run records them on every n-th step)
    c->timing_now = (c->timing && c->timing_steps++ % c->timing_period == 0) ? c->timing : 0;
    if (c->timing_now) {
        make_events(c);
        c->tset = (int)(c->timed_steps & 1);
        collect_timing(c, c->tset);          // (the set's last use is two timed steps old: this returns at once)
    }
}

static int enq_init_iframe(psamd_ctx *c)
{
    tick(c, psamd_ctx::E_RESET);
    // cell / chunk / queue-record counts and the per-frame scalars (the sticky error word stays): the last kernel of
    // the step before did it, unless there was none
    if (!c->frame_clean) PS_HIP(c, launch_frame_reset(c->stream, c->d, c->frame_ints, c->P.world > 1 ? 4 * c->geo.num_chunks : 0));
    return PSAMD_OK;
}

static uint64_t build_key(const psamd_ctx *c) { return (c->frame_clean ? 0ull : 1ull) | (c->tdata_mirror ? 2ull : 0ull) | (c->ledger.big_cells() ? 4ull : 0ull); }

static int enq_build_grid(psamd_ctx *c)
{
    PS_HIP(c, launch_build_grid(c->stream, c->P, c->d, c->timing_now >= 2 ? &c->ev[c->tset][psamd_ctx::E_HIST] : nullptr, c->tdata_mirror, c->ledger.big_cells()));
    return PSAMD_OK;
}

static int64_t alive_at_most(const psamd_ctx *c) { return c->ledger.alive_at_most(ledger_params(c), c->graphs); }
static int64_t pairs_hint(const psamd_ctx *c, const DevParams &P) { return c->ledger.pairs_hint(ledger_params(c), comp_count(P)); }
static uint64_t bucket_key(const psamd_ctx *c) { return c->ledger.bucket_key(ledger_params(c)); }

static int enq_pairs(psamd_ctx *c, const DevParams &P, int64_t tasks_hint, bool last = true, bool first = true)
{
    if (first) tick(c, psamd_ctx::E_COLLIDE);
    c->pairs_shape_last = launch_pairs_shape(P, tasks_hint);
    PS_HIP(c, launch_pairs(c->stream, P, c->d, (c->timing_now && first) ? c->ev[c->tset][psamd_ctx::E_FORCE] : nullptr, tasks_hint, first ? 0 : 1, alive_at_most(c)));
    if (last) tick(c, psamd_ctx::E_PAIRS_END);
    return PSAMD_OK;
}

// kill / survive / integrate / explosion for every own particle; in slab mode the particles
// that leave for a neighbour's segment are in the outboxes when this has run
static int enq_apply(psamd_ctx *c, int64_t bound)
{
    tick(c, psamd_ctx::E_APPLY);
    PS_HIP(c, launch_apply(c->stream, c->P, c->S, c->d));
    const SlabMsg *m = c->msg;       // the outboxes: below, above, two below, two above, far
    int *const out[5] = {m[MSG_XFER_OUT].ptr, m[MSG_XFER_OUT + 1].ptr, m[MSG_XFER2_OUT].ptr, m[MSG_XFER2_OUT + 1].ptr, m[MSG_FAR_OUT].ptr};
    if (c->P.world > 1) PS_HIP(c, launch_outbox_close(c->stream, c->P, c->d, bound, out));
    return PSAMD_OK;
}

// free-slot queues and relocation (in slab mode: after the arrivals were merged in): census, bucketing -- the last
// bucketing workgroup hands the step's scalars to the host's pinned record --, replay + commit; the last launch
// is also the next frame's init_iframe
static int enq_lifecycle(psamd_ctx *c, int64_t bound)
{
    tick(c, psamd_ctx::E_LIFE);
    const SlabMsg *m = c->msg;
    const int *const in[5] = {m[MSG_XFER_IN].ptr, m[MSG_XFER_IN + 1].ptr, m[MSG_XFER2_IN].ptr, m[MSG_XFER2_IN + 1].ptr, m[MSG_FAR_IN].ptr};
    if (c->P.world > 1) PS_HIP(c, launch_inbox_merge(c->stream, c->P, c->d, in));
    PS_HIP(c, launch_lifecycle(c->stream, c->P, c->d, c->geo.queue_infos, StepLedger::lifecycle_bound(ledger_params(c), bound), c->ledger.bucket_cap(ledger_params(c)),
                               c->frame_ints, c->P.world > 1 ? 4 * c->geo.num_chunks : 0));
    tick(c, psamd_ctx::E_END);
    return PSAMD_OK;
}

// ---- hipGraph cache ----
void psamd::drop_graphs(psamd_ctx *c)
{
    for (auto &cache : c->gcache) {
        for (auto &g : cache) if (g.exec) (void)hipGraphExecDestroy(g.exec);
        cache.clear();
    }
}

template <typename F>
static int run_segment(psamd_ctx *c, int seg, uint64_t key, F enqueue)
{
    if (!c->graphs || c->timing_now) return enqueue();
    auto &cache = c->gcache[seg];
    for (auto &g : cache)
        if (g.key == key) {
            g.stamp = ++c->gstamp;
            PS_HIP(c, hipGraphLaunch(g.exec, c->stream));
            c->graph_launches++;
            return PSAMD_OK;
        }
    // not seen with this shape: capture the sequence once, then replay it
    hipError_t e = hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed);
    if (e == hipSuccess) {
        const int rc = enqueue();
        hipGraph_t graph = nullptr;
        e = hipStreamEndCapture(c->stream, &graph);
        hipGraphExec_t exec = nullptr;
        if (rc == PSAMD_OK && e == hipSuccess && graph) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (graph) (void)hipGraphDestroy(graph);
        if (rc != PSAMD_OK) return rc;
        if (e == hipSuccess && exec) {
            if (cache.size() >= 8) {                      // the shape that was used longest ago makes room
                size_t old = 0;
                for (size_t k = 1; k < cache.size(); k++) if (cache[k].stamp < cache[old].stamp) old = k;
                (void)hipGraphExecDestroy(cache[old].exec);
                cache.erase(cache.begin() + (long)old);
            }
            cache.push_back({key, exec, ++c->gstamp});
            c->graph_captures++;
            PS_HIP(c, hipGraphLaunch(exec, c->stream));
            c->graph_launches++;
            return PSAMD_OK;
        }
    }
    // the runtime would not capture this: the context goes on without graphs (nothing was executed so far)
    (void)hipGetLastError();
    c->graphs = false;
    c->graph_refused = std::string(hipGetErrorString(e));
    return enqueue();
}

// The host's and the device's count of the scalar records part ways if a launch fails between the kernel that
// publishes a record and the host's bookkeeping of the step: after an error both are set to what the device holds.
static void resync_scalars(psamd_ctx *c)
{
    if (hipStreamSynchronize(c->stream) != hipSuccess) return;
    StepState st{};
    if (hipMemcpy(&st, c->d.st, sizeof st, hipMemcpyDeviceToHost) != hipSuccess) return;
    c->ledger.resync(st.seq);
}

// Wait until the scalars of step `seq` are in the host's record: the publishing workgroup stores the record's
// number last.  The stream is looked at now and then so that a failed launch cannot leave the host waiting, and
// the wall clock too: a stream that stays busy without ever publishing is a wedged GPU, reported as such
// (PSAMD_ERR_STATE, sticky) instead of a host thread that never comes back.
// Policy 0 spins on the word (lowest latency); policy 1, the default of a slab, spins for a few microseconds and
// then sleeps in short naps -- eight ranks of a node do not pin eight cores for the whole run.  The naps need a
// timer slack of ~1 us (the default 50 us would BE the nap): set for the wait, restored before it returns.
static int wait_scalars(psamd_ctx *c, int seq)
{
    volatile int32_t *word = &c->h_fs[seq & 1].seq;
    if (*word == seq) { std::atomic_thread_fence(std::memory_order_acquire); return PSAMD_OK; }
    const bool naps = c->wait_policy == 1;
    long old_slack = -1;
    int rc = PSAMD_OK;
    struct timespec t0;
    (void)clock_gettime(CLOCK_MONOTONIC, &t0);
    for (uint64_t spins = 1; *word != seq; spins++) {
        if (naps && spins > 2000) {
            if (old_slack < 0) { old_slack = prctl(PR_GET_TIMERSLACK, 0UL, 0UL, 0UL, 0UL); (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0UL, 0UL, 0UL); }
            struct timespec ts = {0, 5000};
            (void)nanosleep(&ts, nullptr);
        } else
            __builtin_ia32_pause();
        if ((spins & (naps ? 0x3ff : 0x3fff)) == 0) {
            const hipError_t e = hipStreamQuery(c->stream);
            if (e == hipSuccess) {
                if (*word == seq) break;
                rc = fail(c, PSAMD_ERR_STATE, "the step's scalars never arrived on the host");
                break;
            }
            if (e != hipErrorNotReady) { rc = hip_fail(c, e, "waiting for the step's scalars"); break; }
            struct timespec t1;
            (void)clock_gettime(CLOCK_MONOTONIC, &t1);
            if ((double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec) > c->wait_limit_s) { c->wedged = true; rc = refuse_wedged(c); break; }
        }
    }
    if (old_slack >= 0) (void)prctl(PR_SET_TIMERSLACK, (unsigned long)old_slack, 0UL, 0UL, 0UL);
    std::atomic_thread_fence(std::memory_order_acquire);
    return rc;
}

// Read the records of the steps up to number `upto` (waiting for them) and whatever has arrived beyond; the first
// verdict met is held for the call that reports it.
static int consume_scalars(psamd_ctx *c, int upto)
{
    StepLedger &L = c->ledger;
    int verdict = PSAMD_OK;
    while (L.seen() < L.seq()) {
        const int s = L.seen() + 1;
        if (s <= upto) { const int st = wait_scalars(c, s); if (st != PSAMD_OK) { if (!c->wedged) resync_scalars(c); return st; } }
        else if (*(volatile int32_t *)&c->h_fs[s & 1].seq != s) break;
        std::atomic_thread_fence(std::memory_order_acquire);
        const FrameScalars r = c->h_fs[s & 1];
        if (L.absorb(r, ledger_params(c), verdict != PSAMD_OK)) verdict = check_device_errors(c);
    }
    L.hold_verdict(verdict, c->err);
    return PSAMD_OK;
}

static int take_verdict(psamd_ctx *c) { return c->ledger.take_verdict(c->err); }

// the rest of the step, once enq_lifecycle is enqueued (or replayed): the host's bookkeeping
static int finish_step(psamd_ctx *c)
{
    c->host_queues_valid = false;
    c->ledger.enqueued();
    if (c->timing_now) { c->ev_level[c->tset] = c->timing_now; c->timed_steps++; }
    c->frame_clean = true;                       // (the step's last kernel zeroed the counts for the frame that follows)
    c->step++; c->steps_total++;
    const int rc = consume_scalars(c, c->ledger.due());
    return rc != PSAMD_OK ? rc : take_verdict(c);
}

// everything enqueued so far has run: read every record outstanding (psamd_synchronize and the calls that hand
// state or counters to the caller)
int psamd::drain_scalars(psamd_ctx *c, bool quiet)
{
    PS_HIP(c, hipStreamSynchronize(c->stream));
    const int rc = consume_scalars(c, c->ledger.seq());
    return rc != PSAMD_OK ? rc : quiet ? (int)PSAMD_OK : take_verdict(c);
}

extern "C" {

int psamd_init_iframe(psamd_ctx *c)
{
    PS_TRY(enter_stage(c, CALL_INIT_IFRAME));
    begin_step(c);
    if (built(c->stage)) c->frame_clean = false;      // (a frame abandoned after its build: its counts are in the way)
    PS_TRY(enq_init_iframe(c));
    c->frame_clean = true;
    leave(c->stage, CALL_INIT_IFRAME);
    return PSAMD_OK;
}

int psamd_build_grid(psamd_ctx *c)
{
    PS_TRY(enter_stage(c, CALL_BUILD_GRID));
    PS_TRY(enq_build_grid(c));
    c->frame_clean = false;
    leave(c->stage, CALL_BUILD_GRID);
    return PSAMD_OK;
}

int psamd_calc_forces_pairs(psamd_ctx *c)
{
    PS_TRY(enter_stage(c, CALL_PAIRS));
    PS_TRY(enq_pairs(c, c->P, pairs_hint(c, c->P)));
    leave(c->stage, CALL_PAIRS);
    return PSAMD_OK;
}

int psamd_calc_forces_apply(psamd_ctx *c)
{
    PS_TRY(enter_stage(c, CALL_APPLY));
    const int64_t bound = alive_at_most(c);
    int rc = enq_apply(c, bound);
    if (rc == PSAMD_OK) rc = enq_lifecycle(c, bound);
    if (rc != PSAMD_OK) { resync_scalars(c); return rc; }
    leave(c->stage, CALL_APPLY);
    return finish_step(c);
}

int psamd_calc_forces(psamd_ctx *c)
{
    PS_TRY(psamd_calc_forces_pairs(c));
    return psamd_calc_forces_apply(c);
}

int psamd_step(psamd_ctx *c, int32_t nsteps)
{
    if (!c || nsteps < 0) return PSAMD_ERR_INVALID_ARG;
    if (nsteps == 0) return c->wedged ? refuse_wedged(c) : (int)PSAMD_OK;
    for (int k = 0; k < nsteps; k++) {
        // init_iframe, build_grid, calc_forces: one sequence of launches (one graph)
        PS_TRY(enter_stage(c, CALL_STEP));
        begin_step(c);
        if (built(c->stage)) c->frame_clean = false;
        const int64_t hint = pairs_hint(c, c->P), bound = alive_at_most(c);
        const uint64_t key = launch_pairs_shape(c->P, hint) | ((uint64_t)bound << 24) | bucket_key(c) | (build_key(c) << 58);
        int rc = run_segment(c, SEG_STEP, key, [&]() {
            int r = enq_init_iframe(c);
            if (r == PSAMD_OK) r = enq_build_grid(c);
            if (r == PSAMD_OK) r = enq_pairs(c, c->P, hint);
            if (r == PSAMD_OK) r = enq_apply(c, bound);
            if (r == PSAMD_OK) r = enq_lifecycle(c, bound);
            return r;
        });
        c->frame_clean = false;
        if (rc != PSAMD_OK) { resync_scalars(c); return rc; }
        leave(c->stage, CALL_STEP);
        PS_TRY(finish_step(c));
    }
    return PSAMD_OK;
}

// ---- slab stages: the step cut where neighbouring ranks exchange messages -----------------

int psamd_slab_build(psamd_ctx *c)
{
    PS_TRY(enter_stage(c, CALL_SLAB_BUILD));
    begin_step(c);
    if (built(c->stage)) c->frame_clean = false;
    // the transfer messages' capacity in force from this step on: both ends of every message change size in the same step
    if (const int cap = c->ledger.adopt_cap(ledger_params(c)); cap != c->P.xfer_cap) {
        c->P.xfer_cap = c->P_int.xfer_cap = c->P_rest.xfer_cap = cap;
        for (int k = MSG_XFER_OUT; k < MSG_XFER_IN + 2; k++) c->msg[k].bytes = xfer_msg_bytes((size_t)cap + 1);
    }
    const int rc = run_segment(c, SEG_BUILD, build_key(c), [&]() {
        int r = enq_init_iframe(c);
        if (r == PSAMD_OK) r = enq_build_grid(c);
        if (r != PSAMD_OK) return r;
        // what is all-gathered before the pair stage: the own snapshot (all-pairs) or the own cells' fp64 sums (a far slab)
        if (c->msg[MSG_ALLG_OUT].ptr)
            PS_HIP(c, far_context(c->P.flags) ? launch_far_own_sums(c->stream, c->P, c->d, c->msg[MSG_ALLG_OUT].ptr)
                                        : launch_allg_pack(c->stream, c->P, c->d, c->msg[MSG_ALLG_OUT].ptr));
        int *const halo_out[2] = {c->msg[MSG_HALO_OUT].ptr, c->msg[MSG_HALO_OUT + 1].ptr};
        if (c->P.world > 1) PS_HIP(c, launch_pack_halos(c->stream, c->P, c->d, c->halo_out_c0, c->halo_out_cells, halo_out, c->pack_off));
        return (int)PSAMD_OK;
    });
    if (rc != PSAMD_OK) return rc;
    c->frame_clean = false;
    leave(c->stage, CALL_SLAB_BUILD);
    return PSAMD_OK;
}

// optional, between slab_build and the arrival of the halo: the pair stage of the cells whose
// stencil lies inside this rank's own layers
int psamd_slab_pairs_interior(psamd_ctx *c)
{
    PS_TRY(enter_stage(c, CALL_SLAB_INTERIOR));
    if (!c->have_interior || interior_passed(c->stage)) return PSAMD_OK;
    const int64_t hint = pairs_hint(c, c->P_int);
    const int rc = run_segment(c, SEG_PAIRS, launch_pairs_shape(c->P_int, hint) | (1ull << 40), [&]() {
        // (the status records have landed: the chunk lists' capacity rule over all ranks decides which particles the stage leaves alone)
        PS_HIP(c, launch_chunk_census(c->stream, c->P, c->d, c->msg[MSG_STATUS_IN].ptr));
        return enq_pairs(c, c->P_int, hint, false, true);
    });
    if (rc != PSAMD_OK) return rc;
    c->ledger.interior_pass_ran();
    leave(c->stage, CALL_SLAB_INTERIOR);
    return PSAMD_OK;
}

int psamd_slab_pairs(psamd_ctx *c)
{
    PS_TRY(enter_stage(c, CALL_SLAB_PAIRS));
    const DevParams &P = c->P;
    const bool second = interior_passed(c->stage);
    const DevParams &Pp = second ? c->P_rest : c->P;
    const int64_t hint = pairs_hint(c, Pp);
    // (the all-pairs far pass sizes its launch from the live bound on one GPU only -- a slab takes every entry of the
    // sorted order, see launch_pairs -- so the bound is no part of this key)
    const int rc = run_segment(c, SEG_PAIRS, launch_pairs_shape(Pp, hint) | (second ? 2ull << 40 : 0ull), [&]() {
        const int GG = P.G * P.G;
        // from the rank below: halo layer (region 1), then lent layers (region 2); from the rank above: halo layer (region 3)
        PS_HIP(c, launch_unpack_halos(c->stream, P, c->d, c->halo_in_cells[0], c->msg[MSG_HALO_IN].ptr, c->unpack_off[0],
                                      c->halo_in_cells[1], c->msg[MSG_HALO_IN + 1].ptr, c->unpack_off[1]));
        // all-pairs: the gathered snapshot, by global cell; a far slab: the gathered cell sums become the moments of the whole box
        if (c->msg[MSG_ALLG_IN].ptr) PS_HIP(c, far_context(P.flags) ? launch_far_gathered(c->stream, P, c->d) : launch_allg_index(c->stream, P, c->d));
        // the chunk lists' capacity rule over all ranks (the status records have landed): which particles the step leaves alone
        if (!second) PS_HIP(c, launch_chunk_census(c->stream, P, c->d, c->msg[MSG_STATUS_IN].ptr));
        const int r = enq_pairs(c, Pp, hint, true, !second);
        if (r != PSAMD_OK) return r;
        if (c->msg[MSG_FORCE_OUT].ptr) PS_HIP(c, launch_pack_force(c->stream, P, c->d, c->msg[MSG_FORCE_OUT].ptr, P.reg_layers[2] * GG * P.halo_cap_cell));
        return (int)PSAMD_OK;
    });
    leave(c->stage, CALL_SLAB_PAIRS, rc == PSAMD_OK);      // (the interior pass is spent either way)
    return rc;
}

int psamd_slab_apply(psamd_ctx *c)
{
    PS_TRY(enter_stage(c, CALL_SLAB_APPLY));
    const int64_t bound = alive_at_most(c);
    const int rc = run_segment(c, SEG_APPLY, (uint64_t)bound | ((uint64_t)c->P.xfer_cap << 32), [&]() {
        // the status records of all ranks (all-gathered since slab_build): error bits, cell-overflow kills for the
        // owner of queue record 0, the transfer messages' next capacity; in
        // the same launch the force records of the lent-out layers (the tail of the snapshot that went up)
        PS_HIP(c, launch_status_merge(c->stream, c->P, c->d, c->msg[MSG_STATUS_IN].ptr, c->halo_out_cells[1] - (c->P.lentout_c1 - c->P.lentout_c0),
                                      c->msg[MSG_FORCE_IN].ptr, c->pack_off[1]));
        return enq_apply(c, bound);
    });
    if (rc != PSAMD_OK) return rc;
    c->slab_bound = bound;
    leave(c->stage, CALL_SLAB_APPLY);
    return PSAMD_OK;
}

int psamd_slab_finish(psamd_ctx *c)
{
    PS_TRY(enter_stage(c, CALL_SLAB_FINISH));
    leave(c->stage, CALL_SLAB_FINISH);           // (the slab frame is over whatever becomes of the launches)
    const int64_t bound = c->slab_bound;
    const int rc = run_segment(c, SEG_FINISH, (uint64_t)bound | ((uint64_t)(c->P.xfer_cap & 0x1fffffff) << 32) | bucket_key(c), [&]() { return enq_lifecycle(c, bound); });
    if (rc != PSAMD_OK) { resync_scalars(c); return rc; }
    return finish_step(c);
}

int psamd_synchronize(psamd_ctx *c)
{
    if (!c) return PSAMD_ERR_INVALID_ARG;
    const int rc = drain_scalars(c);             // (the verdict of every step whose record had not been read yet)
    if (rc != PSAMD_OK) return rc;
    return check_device_errors(c);
}

int psamd_set_stream(psamd_ctx *c, void *hip_stream)
{
    if (!c) return PSAMD_ERR_INVALID_ARG;
    PS_HIP(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return PSAMD_OK;
}

int psamd_get_stream(psamd_ctx *c, void **out)
{
    if (!c || !out) return PSAMD_ERR_INVALID_ARG;
    *out = (void *)c->stream;
    return PSAMD_OK;
}

int psamd_set_graphs(psamd_ctx *c, int enabled)
{
    if (!c) return PSAMD_ERR_INVALID_ARG;
    PS_HIP(c, hipStreamSynchronize(c->stream));
    if (!enabled) drop_graphs(c);
    c->graphs = enabled != 0;
    c->graph_refused.clear();
    return PSAMD_OK;
}

int psamd_get_graph_stats(psamd_ctx *c, int64_t *launches, int64_t *captures)
{
    if (!c) return PSAMD_ERR_INVALID_ARG;
    if (launches) *launches = c->graph_launches;
    if (captures) *captures = c->graph_captures;
    if (!c->graph_refused.empty()) return fail(c, PSAMD_ERR_UNSUPPORTED, "the HIP runtime would not capture a stage sequence (" + c->graph_refused + "); the context runs without graphs");
    return PSAMD_OK;
}

int psamd_set_wait_policy(psamd_ctx *c, int policy)
{
    if (!c || policy < 0 || policy > 1) return PSAMD_ERR_INVALID_ARG;
    c->wait_policy = policy;
    return PSAMD_OK;
}

int psamd_set_tdata_mirror(psamd_ctx *c, int enabled)
{
    if (!c) return PSAMD_ERR_INVALID_ARG;
    c->tdata_mirror = enabled != 0;
    return PSAMD_OK;
}

int psamd_set_run_ahead(psamd_ctx *c, int steps)
{
    if (!c || steps < 0 || steps > 1) return PSAMD_ERR_INVALID_ARG;
    c->ledger.set_run_ahead(steps);
    return PSAMD_OK;
}

int psamd_set_timing(psamd_ctx *c, int enabled)
{
    if (!c) return PSAMD_ERR_INVALID_ARG;
    collect_timing(c, 0); collect_timing(c, 1);          // (whatever is outstanding belongs to the setting that ends here)
    c->timing = enabled < 0 ? 0 : enabled > 2 ? 2 : enabled;
    c->timing_steps = 0; c->timing_now = 0;
    if (c->timing) make_events(c);
    for (double &v : c->t_us) v = 0.0;
    for (auto &v : c->t_samples) v.clear();
    c->t_launches = 0;
    return PSAMD_OK;
}

int psamd_set_timing_period(psamd_ctx *c, int every)
{
    if (!c || every < 1) return PSAMD_ERR_INVALID_ARG;
    c->timing_period = every;
    c->timing_steps = 0;
    return PSAMD_OK;
}

int psamd_get_timing(psamd_ctx *c, double us_out[PSAMD_NUM_TIMERS], int64_t *launches)
{
    if (!c || !us_out) return PSAMD_ERR_INVALID_ARG;
    collect_timing(c, 0); collect_timing(c, 1);
    for (int k = 0; k < PSAMD_NUM_TIMERS; k++) us_out[k] = c->t_us[k];
    if (launches) *launches = c->t_launches;
    return PSAMD_OK;
}

int psamd_get_timing_stats(psamd_ctx *c, double median_us[PSAMD_NUM_TIMERS], double max_us[PSAMD_NUM_TIMERS], int64_t *samples)
{
    if (!c || !median_us || !max_us) return PSAMD_ERR_INVALID_ARG;
    collect_timing(c, 0); collect_timing(c, 1);
    for (int k = 0; k < PSAMD_NUM_TIMERS; k++) {
        std::vector<float> v = c->t_samples[k];
        median_us[k] = max_us[k] = 0.0;
        if (v.empty()) continue;
        std::sort(v.begin(), v.end());
        median_us[k] = v[v.size() / 2]; max_us[k] = v.back();
    }
    if (samples) *samples = c->t_launches;
    return PSAMD_OK;
}

}  // extern "C"
