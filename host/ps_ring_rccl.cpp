// ps_ring_rccl.cpp -- the multi-GPU step in C++: libpsamd.so's four slab stage calls with the
// messages moved by RCCL (ncclSend / ncclRecv / ncclAllGather) straight between the contexts'
// device buffers.  No Python, no torch: include/psamd.h, the HIP runtime and rccl.h.  This is
// what the reference's pmlib layer does for it between nodes (subscriptions to segments,
// ps.cpp:380-487; the stage loop, ps.cpp:1843-1928); here one process drives one GPU.
//
//   one process per GPU (what a node runs; bench.py --gpus N starts these):
//       ps_ring_rccl --world W --rank r --device d --id-file /tmp/id --job J [--bench ...]
//     rank 0 writes the communicator's ncclUniqueId to the file (tagged with the job's nonce J), the others wait for it.
//   all slabs in ONE process on GPU 0 (what a one-GPU test box can run):
//       ps_ring_rccl --world W --loopback [--n N] [--iters K] [--seed S] [--all-pairs | --far flat|pyramid|quadrupole] [--births]
//     The communicator has a single rank; every message is an ncclSend to self matched by
//     an ncclRecv from self in the same group -- RCCL moves every byte, between the buffers of
//     different contexts.  This mode also runs the whole system in one plain context and
//     requires the union of the slabs to equal it byte for byte (P_DATA_TYPE of every slot).
//   without a GPU (tests): --id-only, --launch-check (the rendezvous), --routes (the route table of one rank).
//
// The parts: ring_routes.hpp -- which messages exist, between whom, in which buffers: one table that the sends, the
// receives and the size check all derive from; ring_step.hpp -- one step: the stage calls, the exchange, the streams and
// events; ring_bench.hpp -- the benchmark protocol and its record; ring_options.hpp -- the command line.  Here: the
// rendezvous, the hooks that need no GPU, making the slabs, the plain run with its loopback check, the teardown.
// Both modes post their messages through the same exchange(): loopback differs only in which slabs are local and in that
// every peer is communicator rank 0.
#include <cstring>

#include "ring_bench.hpp"

namespace {

// The id file carries the job's nonce (--job, the same on every rank of one job) in front of the id: a file
// left behind by an earlier job is not this job's and is waited past, not read.  Rank 0 removes whatever is
// there before it writes (tmp + rename: never a half-written file) and again once the communicator is up.
struct IdFile { uint64_t magic, job; ncclUniqueId id; };
const uint64_t kMagic = 0x70735f72696e6731ull;        // "ps_ring1"

// the communicator's id on every rank: communicator rank 0 makes it (without a GPU: from the job's nonce) and writes the file, the others wait for it
int rendezvous(const Options &o, bool no_gpu, ncclUniqueId *id)
{
    if (o.loopback || o.rank == 0) {
        if (no_gpu) { uint64_t x = o.job * 0x9E3779B97F4A7C15ull + 1; for (size_t i = 0; i < sizeof *id; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; ((char *)id)[i] = (char)x; } }
        else NCCL_OK(ncclGetUniqueId(id));
        if (o.id_file.empty()) return 0;
        std::remove(o.id_file.c_str());
        IdFile rec{kMagic, o.job, *id};
        std::ofstream f(o.id_file + ".tmp", std::ios::binary);
        f.write((const char *)&rec, sizeof rec);
        f.close();
        if (!f || std::rename((o.id_file + ".tmp").c_str(), o.id_file.c_str()) != 0) { std::fprintf(stderr, "cannot write %s\n", o.id_file.c_str()); return 1; }
        return 0;
    }
    for (int tries = 0;; tries++) {
        IdFile rec{};
        std::ifstream f(o.id_file, std::ios::binary);
        if (f && f.read((char *)&rec, sizeof rec) && rec.magic == kMagic && rec.job == o.job) { *id = rec.id; return 0; }
        if (tries > 600) { std::fprintf(stderr, "no communicator id of job %llu in %s\n", (unsigned long long)o.job, o.id_file.c_str()); return 1; }
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
    }
}

// --routes: the route table of one rank, as the exchange derives its sends and receives from it (tests hold it against slab.py)
int print_routes(const Options &o)
{
    for (const Route &m : routes(o.rank, o.world)) std::printf("send %s %d %d %d %d %d\n", kPhaseName[m.phase], m.out_slot, m.peer, m.in_slot, m.hop, m.dir);
    for (const Route &m : receives(o.rank, o.world)) std::printf("recv %s %d %d %d %d %d\n", kPhaseName[m.phase], m.out_slot, m.peer, m.in_slot, m.hop, m.dir);
    return 0;
}

// --launch-check: every rank reports in through a file beside the id file; rank 0 waits for all of them and
// prints the skeleton of the benchmark record -- proves bench.py's launcher of C++ ranks on a machine without GPUs
int launch_check(const Options &o, unsigned sum)
{
    auto file_of = [&](int r) { return o.id_file + ".in" + std::to_string(r); };
    { std::ofstream f(file_of(o.rank), std::ios::binary); f << sum << " " << o.job << "\n"; }
    if (o.rank != 0) return 0;
    int seen = 0;
    for (int tries = 0; tries < 600 && seen < o.world; tries++) {
        seen = 0;
        for (int r = 0; r < o.world; r++) {
            std::ifstream f(file_of(r));
            unsigned s2 = 0; unsigned long long j2 = 0;
            if (f && (f >> s2 >> j2) && s2 == sum && j2 == o.job) seen++;
        }
        if (seen < o.world) std::this_thread::sleep_for(std::chrono::milliseconds(100));
    }
    for (int r = 0; r < o.world; r++) std::remove(file_of(r).c_str());
    std::remove(o.id_file.c_str());
    if (seen < o.world) { std::fprintf(stderr, "launch check: %d of %d ranks reported in\n", seen, o.world); return 1; }
    std::printf("{\"psamd_ring\": 1, \"launch_check\": true, \"world\": %d, \"steps\": %d, \"warmup\": %d}\n", seen, o.steps, o.warmup);
    return 0;
}

// (test hooks: the rendezvous through the file, without a GPU or RCCL transport)
int run_without_gpu(const Options &o)
{
    ncclUniqueId id;
    if (rendezvous(o, true, &id)) return 1;
    unsigned sum = 0;
    for (size_t i = 0; i < sizeof id; i++) sum = sum * 131u + (unsigned char)((const char *)&id)[i];
    if (o.launch_check) return launch_check(o, sum);
    std::printf("rank %d of %d: communicator id %08x (job %llu)\n", o.rank, o.world, sum, (unsigned long long)o.job);
    return 0;
}

// the particles every slab is shown (each keeps its own segments'), and the configuration they share
struct Cloud { psamd_config cfg0; std::vector<float> xyz, age, fert; };

// --far: the far-field force model of the slabs and of the loopback check's plain context.  The slabs also say that this host
// all-gathers the cell sums (PSAMD_FLAG_FAR_SLAB: allg_out into allg_in between slab_build and slab_pairs, ring_step.hpp)
uint32_t far_flags(const Options &o)
{
    const uint32_t model[4] = {0u, PSAMD_FLAG_FAR_MONOPOLE, PSAMD_FLAG_FAR_PYRAMID, PSAMD_FLAG_FAR_PYRAMID | PSAMD_FLAG_FAR_QUADRUPOLE};
    return model[far_model(o)];
}

void make_config(const Options &o, psamd_config *cfg0)
{
    psamd_default_config(cfg0);
    cfg0->chunk_factor = o.chunk_factor; cfg0->chunk_dim = o.chunk_dim;
    cfg0->max_particles_num = (int32_t)std::max<int64_t>(std::max<int64_t>(o.n, o.max_particles), 1 << 20);
    cfg0->flags = (o.all_pairs ? PSAMD_FLAG_ALL_PAIRS : 0u) | (o.births ? PSAMD_FLAG_EXPLOSIONS : 0u) | (o.fast_math ? PSAMD_FLAG_FAST_MATH : 0u) | far_flags(o);
    cfg0->halo_cap_cell = o.halo_cap_cell; cfg0->xfer_cap = o.xfer_cap;
    cfg0->seed = o.seed;
}

// a uniform cloud; ages of adults [MIN_ADULT_AGE, MAX_ADULT_AGE); births: fertility ages they reach within a few steps
int make_cloud(const Options &o, psamd_ctx *ctx, Cloud &c)
{
    const double life = c.cfg0.life_steps * c.cfg0.dt;
    c.xyz.resize((size_t)3 * o.n); c.age.resize((size_t)o.n); c.fert.resize((size_t)o.n);
    PS_OK(ctx, psamd_uniform_cloud(ctx, o.n, o.seed, c.xyz.data()));
    uint64_t x = o.seed * 0x9E3779B97F4A7C15ull + 1;
    for (int64_t i = 0; i < o.n; i++) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        const double u = (double)(x >> 40) * (1.0 / 16777216.0);
        c.age[(size_t)i] = (float)(life / 7.0 + (life / 2.0 - life / 7.0) * u);
        c.fert[(size_t)i] = o.births ? (float)(c.age[(size_t)i] + c.cfg0.dt * (double)(1 + (x & 15))) : 1.0e6f + (float)(o.bench ? 0 : i);
    }
    return 0;
}

// the slabs this process holds, all shown the same particles
int make_slabs(Ring &R, const Options &o, Cloud &cloud)
{
    for (int r = 0; r < o.world; r++) {
        if (!o.loopback && r != o.rank) continue;
        Slab s; s.rank = r;
        psamd_config cfg = cloud.cfg0;
        cfg.device = o.device; cfg.rank = r; cfg.world = o.world;
        if (far_flags(o)) cfg.flags |= PSAMD_FLAG_FAR_SLAB;
        if (o.break_sizes && r == 1) cfg.halo_cap_cell = (cfg.halo_cap_cell > 0 ? cfg.halo_cap_cell : 64) + 8;
        psamd_ctx *ctx = nullptr;
        PS_OK(ctx, psamd_create(&cfg, &ctx));
        s.ctx = ctx;
        if (R.local.empty() && make_cloud(o, ctx, cloud)) return 1;
        PS_OK(ctx, psamd_fill_particles(ctx, o.n, cloud.xyz.data(), nullptr, nullptr, cloud.age.data(), cloud.fert.data(), nullptr, nullptr));
        if (R.local.empty()) {
            // Which stream the stage kernels (and, by default, the RCCL calls) run on: the first context's OWN stream.  Measured
            // (profiles/r5_ab_host.txt): with a stream this program created itself -- before the contexts or after the first
            // one -- a one-rank step takes 0.8-1.2 % longer, all of it inside the force pass's own time; on the context's own
            // stream the C++ host is as fast as the Python host.  Eight slabs in one process: no difference.  The cause is not
            // known (same flags, same kernels, same arguments).
            void *st = nullptr;
            PS_OK(ctx, psamd_get_stream(ctx, &st));
            R.compute = (hipStream_t)st;
            if (!o.side_stream) R.transfer = R.compute;
        }
        PS_OK(ctx, psamd_set_stream(ctx, (void *)R.compute));
        PS_OK(ctx, psamd_set_graphs(ctx, o.graphs ? 1 : 0));
        if (o.bench) PS_OK(ctx, psamd_set_tdata_mirror(ctx, 0));      // (this host never fetches the reference's T_DATA buffer)
        if (o.wait_policy >= 0) PS_OK(ctx, psamd_set_wait_policy(ctx, o.wait_policy));
        PS_OK(ctx, psamd_slab_buffers_get(ctx, &s.b));
        PS_OK(ctx, psamd_get_slab_plan(ctx, &s.plan));
        R.local.push_back(s);
    }
    plan_posts(R);
    return 0;
}

// the device, the transfer stream and the ordering events, the communicator (one rank per process)
int open_ring(Ring &R, const Options &o)
{
    ncclUniqueId id;
    HIP_OK(hipSetDevice(o.device));
    if (o.side_stream) HIP_OK(hipStreamCreateWithFlags(&R.transfer, hipStreamNonBlocking));
    for (hipEvent_t *e : {&R.ev_built, &R.ev_halo, &R.ev_paired, &R.ev_force, &R.ev_applied, &R.ev_xfer}) HIP_OK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    if (rendezvous(o, false, &id)) return 1;
    NCCL_OK(ncclCommInitRank(&R.comm, o.loopback ? 1 : o.world, id, o.loopback ? 0 : o.rank));
    g_comm = R.comm;
    if ((o.loopback || o.rank == 0) && !o.id_file.empty()) std::remove(o.id_file.c_str());      // every rank has joined: the file has served
    return 0;
}

// The contexts in reverse order, the first one last: the others enqueue on its stream.  Then the communicator, then the transfer stream.
void close_ring(Ring &R)
{
    for (size_t i = R.local.size(); i-- > 0;) psamd_destroy(R.local[i].ctx);
    g_comm = nullptr;
    if (R.comm) ncclCommDestroy(R.comm);
    if (R.transfer != R.compute) (void)hipStreamDestroy(R.transfer);
}

struct Particle72 { unsigned char bytes[72]; };

// loopback: the same steps in one plain context: the union of the slabs must be its state
int compare_with_one_context(const Options &o, const Cloud &cloud, const psamd_sizes &sz, const std::vector<Particle72> &merged, bool *same)
{
    std::vector<Particle72> part((size_t)sz.container_size);
    psamd_config cfg = cloud.cfg0;
    cfg.device = o.device;
    psamd_ctx *one = nullptr;
    PS_OK(one, psamd_create(&cfg, &one));
    PS_OK(one, psamd_fill_particles(one, o.n, cloud.xyz.data(), nullptr, nullptr, cloud.age.data(), cloud.fert.data(), nullptr, nullptr));
    PS_OK(one, psamd_set_graphs(one, o.graphs ? 1 : 0));
    PS_OK(one, psamd_step(one, o.iters));
    PS_OK(one, psamd_download_particles(one, part.data(), 0, sz.container_size));
    psamd_counters cn;
    PS_OK(one, psamd_get_counters(one, &cn));
    // free records: a slab reports the slots it does not own as free records, the merge took owned ranges only
    size_t bad = 0;
    for (size_t i = 0; i < merged.size(); i++)
        if (std::memcmp(&merged[i], &part[i], sizeof(Particle72)) != 0) bad++;
    std::printf("ring-rccl %s: %zu of %lld records differ from the single context after %d steps (%lld relocations, %lld births there)\n",
                bad ? "MISMATCH" : "ok", bad, (long long)sz.container_size, o.iters, (long long)cn.relocations, (long long)cn.births);
    *same = bad == 0;
    psamd_destroy(one);
    return 0;
}

// the plain run: --iters steps, a line of figures and, in loopback mode, the check against one context (*same)
int run_plain(Ring &R, const Options &o, const Cloud &cloud, const psamd_sizes &sz, bool *same)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (int it = 0; it < o.iters; it++)
        if (ring_step(R, no_hook)) return 1;
    if (sync_all(R)) return 1;
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    std::vector<Particle72> merged((size_t)sz.container_size), part((size_t)sz.container_size);
    std::memset(merged.data(), 0, merged.size() * sizeof(Particle72));
    int64_t live = 0, replays = 0, captures = 0;
    for (Slab &s : R.local) {
        PS_OK(s.ctx, psamd_download_particles(s.ctx, part.data(), 0, sz.container_size));
        for (int t = 0; t < 4; t++)
            std::memcpy(merged.data() + s.plan.slot_lo[t], part.data() + s.plan.slot_lo[t],
                        (size_t)(s.plan.slot_hi[t] - s.plan.slot_lo[t]) * sizeof(Particle72));
        int64_t l = 0, a = 0, b = 0;
        PS_OK(s.ctx, psamd_live_count(s.ctx, &l));
        PS_OK(s.ctx, psamd_get_graph_stats(s.ctx, &a, &b));       // (an error here: the runtime refused to capture a stage)
        live += l; replays += a; captures += b;
    }
    std::printf("rank %d of %d%s: %d steps, %.1f MB through RCCL, %.3f ms per step, %lld live here, %lld graph replays (%lld captures)%s%s\n", o.rank, o.world,
                o.loopback ? " (all slabs in this process)" : "", o.iters, R.moved / 1e6, 1e3 * secs / std::max(1, o.iters), (long long)live,
                (long long)replays, (long long)captures, o.side_stream == 2 ? ", every transfer on a second stream" : o.side_stream ? ", the status gather (and an overlapped halo) on a second stream" : "",
                o.overlap_interior ? ", interior pass beside the halo" : "");
    *same = true;
    return o.loopback ? compare_with_one_context(o, cloud, sz, merged, same) : 0;
}

}  // namespace

int main(int argc, char **argv)
{
    Options o;
    if (const int rc = parse_args(argc, argv, o)) return rc;
    if (psamd_abi_version() != PSAMD_ABI_VERSION) {
        std::fprintf(stderr, "libpsamd.so has ABI version %d, this program was built against %d: rebuild one of them\n", psamd_abi_version(), PSAMD_ABI_VERSION);
        return 2;
    }
    if (o.routes) return print_routes(o);
    if (o.id_only || o.launch_check) return run_without_gpu(o);

    Ring R;
    R.world = o.world; R.loopback = o.loopback; R.side = o.side_stream; R.overlap_interior = o.overlap_interior;
    Cloud cloud;
    make_config(o, &cloud.cfg0);
    psamd_sizes sz;
    if (open_ring(R, o) || make_slabs(R, o, cloud)) return bail();
    PS_OK(R.local[0].ctx, psamd_get_sizes(R.local[0].ctx, &sz));
    if (check_sizes(R)) return bail();          // every message has the size its receiver expects, or nobody starts

    bool same = true;
    if (o.bench ? run_bench(R, o, sz) : run_plain(R, o, cloud, sz, &same)) return bail();
    close_ring(R);
    return same ? 0 : 1;
}
