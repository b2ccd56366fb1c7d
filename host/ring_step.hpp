// ring_step.hpp -- one step of the slab ring: the four stage calls of every local slab with the messages moved by RCCL
// between them (part of ps_ring_rccl.cpp, which alone includes it).
//
// Two HIP streams.  The stage kernels run on the COMPUTE stream -- with --graphs 1 each stage's kernels as
// one captured hipGraph, so a rank's step is five submissions, not two dozen launches (measured: a graph
// launch costs ~10 us on the GPU's timeline, the plain launches of a host that runs ahead cost nothing:
// profiles/r4_ab_graphs.txt; off by default) --, every RCCL call on the TRANSFER stream; events order the two: the halo (and the all-gather of the all-pairs snapshot blocks or of a far slab's cell sums)
// waits for slab_build and travels while the compute stream runs the interior pair pass (--overlap-interior)
// or simply goes ahead; the all-gather of the status records lands before the first pair-stage call; force and
// transfer messages fork off after slab_pairs / slab_apply and are joined before the stage that reads them.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "psamd.h"
#include "ring_routes.hpp"

namespace {

// A rank that fails must not leave its peers blocked in a receive: abort the communicator on the way out
// (psamd's own failures are collective -- every rank returns the error from the same slab_finish -- but a
// HIP or RCCL error, or a failure during set-up, is not).
ncclComm_t g_comm = nullptr;
int bail() { if (g_comm) { (void)ncclCommAbort(g_comm); g_comm = nullptr; } return 1; }
#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_)); return bail(); } } while (0)
#define NCCL_OK(call) do { ncclResult_t r_ = (call); if (r_ != ncclSuccess) { std::fprintf(stderr, "%s: %s\n", #call, ncclGetErrorString(r_)); return bail(); } } while (0)
#define PS_OK(ctx, call) do { const int rc_ = (call); if (rc_ != PSAMD_OK) { std::fprintf(stderr, "%s failed: %s (%s)\n", #call, psamd_status_string(rc_), (ctx) ? psamd_last_error(ctx) : ""); return bail(); } } while (0)

struct Slab {
    int rank = 0;
    psamd_ctx *ctx = nullptr;
    psamd_slab_buffers b{};
    psamd_slab_plan plan{};
};

// One ncclSend or ncclRecv of this process: a local slab's slot, the communicator rank at the other end, its place in the order
struct Post { size_t slab; int slot, peer; std::array<int, 4> key; };

struct Ring {
    int world = 1;
    bool loopback = false, overlap_interior = false;
    int side = 0;                       // 0: every RCCL call on the compute stream (default); 1: what has compute to travel beside goes on the transfer stream; 2: everything does (round 4)
    ncclComm_t comm = nullptr;
    hipStream_t compute = nullptr;      // the first context's own stream
    hipStream_t transfer = nullptr;     // a stream of this program's (--side-stream 1 or 2), else the compute stream
    hipEvent_t ev_built = nullptr, ev_halo = nullptr, ev_paired = nullptr, ev_force = nullptr, ev_applied = nullptr, ev_xfer = nullptr;
    std::vector<Slab> local;            // the slabs this process holds (one per process in a real run; all of them in loopback mode, where every peer is comm rank 0)
    std::vector<Post> sends[3], recvs[3];       // per phase, in posting order (plan_posts)
    int64_t moved = 0;
    // Stage timing on the compute stream (benchmark runs, every n-th step): per local slab eight events -- before / after
    // each of the four stage calls.  after(stage k) -> before(stage k + 1) is what the compute stream spent WAITING for
    // the phase's messages (the host enqueues the next stage at once; only the event of the transfer stream holds it).
    std::vector<std::vector<hipEvent_t>> stage_ev;      // [timed step][slab * 8 + e]
    int stage_slot = -1;                                // the timed step being recorded, -1: this step carries no events
};

int mark(Ring &R, size_t slab, int e)
{
    if (R.stage_slot < 0) return 0;
    HIP_OK(hipEventRecord(R.stage_ev[(size_t)R.stage_slot][slab * 8 + (size_t)e], R.compute));
    return 0;
}

// every context, the compute stream, the transfer stream: nothing of this process is in flight
int sync_all(Ring &R)
{
    for (Slab &s : R.local) PS_OK(s.ctx, psamd_synchronize(s.ctx));
    HIP_OK(hipStreamSynchronize(R.compute));
    HIP_OK(hipStreamSynchronize(R.transfer));
    return 0;
}

// Every rank's sizes on every rank (all-gathered once; in loopback they are all here), checked against the routes: or nobody starts.
int check_sizes(Ring &R)
{
    std::vector<SizeTable> all((size_t)R.world);
    if (R.loopback) { for (const Slab &s : R.local) all[(size_t)s.rank] = sizes_of(s.b); return sizes_agree(all); }
    if (R.world == 1) return 0;
    SizeTable mine = sizes_of(R.local[0].b), *d = nullptr;
    HIP_OK(hipMalloc((void **)&d, sizeof(SizeTable) * ((size_t)R.world + 1)));
    HIP_OK(hipMemcpyAsync(d + R.world, &mine, sizeof mine, hipMemcpyHostToDevice, R.transfer));
    NCCL_OK(ncclAllGather(d + R.world, d, sizeof(SizeTable), ncclInt8, R.comm, R.transfer));
    HIP_OK(hipMemcpyAsync(all.data(), d, sizeof(SizeTable) * (size_t)R.world, hipMemcpyDeviceToHost, R.transfer));
    HIP_OK(hipStreamSynchronize(R.transfer));
    (void)hipFree(d);
    return sizes_agree(all);
}

// The sends and receives this process may post, per phase: the local slabs' routes and the routes that end at them.  They
// depend on (rank, world) alone, so they are listed once; which of them exist a step decides by the sizes.  Between one
// pair of ranks RCCL matches sends and receives by order alone.  Both lists are ordered by (sender, receiver, hop, direction
// of travel): across processes that is (peer, hop, direction) for a rank's sends and for its receives alike, so its k-th
// send to a peer is that peer's k-th receive from it; in loopback, where every peer is communicator rank 0, the one key
// orders the sends and the receives of all slabs alike, and k-th still meets k-th.
void plan_posts(Ring &R)
{
    for (size_t i = 0; i < R.local.size(); i++) {
        const int r = R.local[i].rank;
        for (const Route &m : routes(r, R.world)) R.sends[m.phase].push_back({i, m.out_slot, R.loopback ? 0 : m.peer, {r, m.peer, m.hop, m.dir}});
        for (const Route &m : receives(r, R.world)) R.recvs[m.phase].push_back({i, m.in_slot, R.loopback ? 0 : m.peer, {m.peer, r, m.hop, m.dir}});
    }
    for (std::vector<Post> *lists : {R.sends, R.recvs})
        for (int ph = 0; ph < 3; ph++) std::sort(lists[ph].begin(), lists[ph].end(), [](const Post &a, const Post &b) { return a.key < b.key; });
}

// One phase's messages as ONE RCCL group on stream `st`: the same body for one slab per process and for loopback
// (a message exists iff its buffer has bytes).
int exchange(Ring &R, Phase ph, hipStream_t st)
{
    auto bytes_of = [&](const std::vector<Post> &v) { int64_t n = 0; for (const Post &p : v) n += buf_of(R.local[p.slab].b, p.slot).bytes; return n; };
    const int64_t out = bytes_of(R.sends[ph]), in = bytes_of(R.recvs[ph]);
    if (!out && !in) return 0;
    // (the transfer messages change size while a run goes on: where both ends are here, a send that no receive would meet is not posted)
    if (R.loopback && out != in) { std::fprintf(stderr, "message sizes disagree: the %s phase sends %lld bytes and receives %lld\n", kPhaseName[ph], (long long)out, (long long)in); return 1; }
    NCCL_OK(ncclGroupStart());
    for (const Post &p : R.sends[ph]) { const Buf m = buf_of(R.local[p.slab].b, p.slot); if (m.bytes) NCCL_OK(ncclSend(m.p, (size_t)m.bytes, ncclInt8, p.peer, R.comm, st)); }
    for (const Post &p : R.recvs[ph]) { const Buf m = buf_of(R.local[p.slab].b, p.slot); if (m.bytes) NCCL_OK(ncclRecv(m.p, (size_t)m.bytes, ncclInt8, p.peer, R.comm, st)); }
    NCCL_OK(ncclGroupEnd());
    R.moved += out;
    return 0;
}

// an all-gathered buffer pair: the status records, the snapshot blocks of an all-pairs run (between slab_build and
// slab_pairs: SURVEY 8(e)'s "all-gather of positions once per step") or in their place the cell sums of a far-field
// run (--far), or the far outboxes of the transfer phase
int gather(Ring &R, int out_slot, int in_slot, hipStream_t st)
{
    const Slab &s0 = R.local[0];
    const size_t nb = (size_t)buf_of(s0.b, out_slot).bytes;
    if (R.world == 1 || !nb) return 0;
    if (!R.loopback) {
        NCCL_OK(ncclAllGather(buf_of(s0.b, out_slot).p, buf_of(s0.b, in_slot).p, nb, ncclInt8, R.comm, st));
        R.moved += (int64_t)nb;
        return 0;
    }
    // a communicator of one rank: its all-gather is a copy; every slab's record into every slab's block
    for (const Slab &src : R.local)
        for (const Slab &dst : R.local)
            NCCL_OK(ncclAllGather(buf_of(src.b, out_slot).p, (char *)buf_of(dst.b, in_slot).p + (size_t)src.rank * nb, nb, ncclInt8, R.comm, st));
    R.moved += (int64_t)nb * (int64_t)R.local.size();
    return 0;
}

// `later` waits for everything enqueued on `earlier` so far (nothing to do when they are one stream)
int order(Ring &R, hipStream_t earlier, hipEvent_t ev, hipStream_t later)
{
    if (earlier == later) return 0;
    HIP_OK(hipEventRecord(ev, earlier));
    HIP_OK(hipStreamWaitEvent(later, ev, 0));
    return 0;
}

// One step of the stage loop (DoParallelProcess, ps.cpp:1843-1928), one slab per GPU.  between(stage): a hook the
// benchmark's frame census uses to read counts back between two stages (nullptr: none).
template <typename Hook>
int ring_step(Ring &R, Hook between)
{
    // Which stream a message travels on.  A dependency that crosses streams costs the GPU's timeline ~15 us each way here
    // (measured, round 5: with every phase on the transfer stream a rank with NO messages at all spent 29 us per phase
    // between two stage kernels -- 88 us of a 720-us rank-step at eight ranks), and pays only where there is compute to
    // travel beside: the halo beside the interior pass, when that is asked for.  The status records must be in before the
    // FIRST pair-stage call (its chunk census decides which particles the stage leaves alone), force and transfer messages
    // before the stage behind them: nothing to travel beside, they go on the compute stream -- an RCCL kernel between two
    // stage kernels, no event.  The default (--side-stream 0) puts EVERYTHING there; 1 is for runs that overlap the halo
    // with the interior pass (--overlap-interior), 2 is round 4's form (every message on the transfer stream), kept for
    // comparison.
    const bool one = R.world == 1;
    hipStream_t s_halo = (R.side == 2 || (R.side == 1 && R.overlap_interior)) ? R.transfer : R.compute;
    hipStream_t s_late = R.side == 2 ? R.transfer : R.compute;      // force, transfer, far outboxes
    for (size_t i = 0; i < R.local.size(); i++) { Slab &s = R.local[i]; if (mark(R, i, 0)) return 1; PS_OK(s.ctx, psamd_slab_build(s.ctx)); if (mark(R, i, 1)) return 1; }
    if (between(0)) return 1;
    if (!one) {
        if (s_halo != R.compute) if (order(R, R.compute, R.ev_built, R.transfer)) return 1;
        if (gather(R, STATUS_OUT, STATUS_IN, s_halo)) return 1;        // first: a 16-KB all-gather, and the interior pass waits for nothing else
        if (s_halo != R.compute) HIP_OK(hipEventRecord(R.ev_force, R.transfer));
        if (exchange(R, HALO, s_halo)) return 1;
        if (gather(R, ALLG_OUT, ALLG_IN, s_halo)) return 1;            // all-pairs forces (the snapshot blocks) and far-field slabs (the cell sums)
        if (s_halo != R.compute) HIP_OK(hipEventRecord(R.ev_halo, R.transfer));
    }
    if (R.overlap_interior) {
        if (!one && s_halo != R.compute) HIP_OK(hipStreamWaitEvent(R.compute, R.ev_force, 0));
        for (Slab &s : R.local) PS_OK(s.ctx, psamd_slab_pairs_interior(s.ctx));      // cells whose stencil lies in the own layers: no halo needed
    }
    if (!one && s_halo != R.compute) HIP_OK(hipStreamWaitEvent(R.compute, R.ev_halo, 0));
    for (size_t i = 0; i < R.local.size(); i++) { Slab &s = R.local[i]; if (mark(R, i, 2)) return 1; PS_OK(s.ctx, psamd_slab_pairs(s.ctx)); if (mark(R, i, 3)) return 1; }
    if (between(1)) return 1;
    if (!one) {
        if (s_late != R.compute) { if (order(R, R.compute, R.ev_paired, R.transfer)) return 1; }
        if (exchange(R, FORCE, s_late)) return 1;
        if (s_late != R.compute) { if (order(R, R.transfer, R.ev_force, R.compute)) return 1; }
    }
    for (size_t i = 0; i < R.local.size(); i++) { Slab &s = R.local[i]; if (mark(R, i, 4)) return 1; PS_OK(s.ctx, psamd_slab_apply(s.ctx)); if (mark(R, i, 5)) return 1; }
    if (!one) {
        // (the transfer messages may have grown: every rank adopts the capacity all of them agreed on two steps ago in the same step)
        for (Slab &s : R.local) PS_OK(s.ctx, psamd_slab_buffers_get(s.ctx, &s.b));
        if (s_late != R.compute) { if (order(R, R.compute, R.ev_applied, R.transfer)) return 1; }
        if (exchange(R, XFER, s_late)) return 1;
        if (gather(R, FAR_OUT, FAR_IN, s_late)) return 1;              // (births on, four or more ranks)
        if (s_late != R.compute) { if (order(R, R.transfer, R.ev_xfer, R.compute)) return 1; }
    }
    for (size_t i = 0; i < R.local.size(); i++) { Slab &s = R.local[i]; if (mark(R, i, 6)) return 1; PS_OK(s.ctx, psamd_slab_finish(s.ctx)); if (mark(R, i, 7)) return 1; }
    return 0;
}
int no_hook(int) { return 0; }

}  // namespace
