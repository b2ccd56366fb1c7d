// ring_bench.hpp -- the benchmark protocol of ps_ring_rccl (--bench; bench.py --gpus N relays the record): census,
// settling steps and warm-up, the timed region, the sustained region, the stage table, the record (part of
// ps_ring_rccl.cpp, which alone includes it).
#pragma once
#include <atomic>
#include <cctype>
#include <chrono>
#include <cstdarg>
#include <fstream>
#include <string>
#include <thread>

#include "ring_options.hpp"
#include "ring_step.hpp"

namespace {

// the shader clock while a timed region runs (sysfs pp_dpm_sclk of the HIP device's PCI function, the level marked current):
// the chip is power-bound under this load, and which clock a figure was taken at is part of the figure
struct ClockWatch {
    std::string path;
    std::vector<int> samples;
    std::atomic<bool> stop{false};
    std::thread th;
    int period_ms = 10;
    explicit ClockWatch(int device, int period = 10) : period_ms(period)
    {
        char bus[64] = {0};
        if (period_ms <= 0) return;
        if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) == hipSuccess) {
            for (char *c = bus; *c; c++) *c = (char)std::tolower((unsigned char)*c);
            path = std::string("/sys/bus/pci/devices/") + bus + "/pp_dpm_sclk";
            std::ifstream f(path);
            if (!f) path.clear();
        }
    }
    void start()
    {
        if (path.empty()) return;
        stop = false;
        th = std::thread([this]() {
            while (!stop) {
                std::ifstream f(path);
                std::string line;
                while (std::getline(f, line)) {
                    if (line.find('*') == std::string::npos) continue;
                    const size_t c = line.find(':');
                    int v = 0;
                    for (size_t i = c == std::string::npos ? 0 : c + 1; i < line.size(); i++) if (std::isdigit((unsigned char)line[i])) v = v * 10 + (line[i] - '0');
                    if (v) samples.push_back(v);
                }
                std::this_thread::sleep_for(std::chrono::milliseconds(period_ms));
            }
        });
    }
    void end() { if (th.joinable()) { stop = true; th.join(); } }
    std::string json()
    {
        if (samples.empty()) return "null";
        std::vector<int> v = samples;
        std::sort(v.begin(), v.end());
        char b[256];
        std::snprintf(b, sizeof b, "{\"min\": %d, \"median\": %d, \"max\": %d, \"samples\": %zu, \"source\": \"%s\"}", v.front(), v[v.size() / 2], v.back(), v.size(), path.c_str());
        return b;
    }
};

// force terms one pair pass evaluates: per visited particle its stencil's population (27 cells, not periodic:
// app.cu:352-409), or -- all-pairs -- every listed body.  A far-field run (--far) counts the stencil's terms only: its far
// bodies, one per cell or per member of the pyramid's far set, are left out, and the record says so (force_terms_count)
double force_terms(const std::vector<int64_t> &n, const std::vector<int32_t> &f, int G, bool all_pairs)
{
    double total = 0;
    if (all_pairs) {
        double sn = 0, sf = 0;
        for (size_t i = 0; i < n.size(); i++) { sn += (double)n[i]; sf += (double)f[i]; }
        return sn * sf;
    }
    for (int i3 = 0; i3 < G; i3++) for (int i1 = 0; i1 < G; i1++) for (int i2 = 0; i2 < G; i2++) {
        const int fc = f[(size_t)(i3 * G + i1) * G + i2];
        if (!fc) continue;
        int64_t nb = 0;
        for (int a = -1; a <= 1; a++) for (int b = -1; b <= 1; b++) for (int d = -1; d <= 1; d++) {
            const int j3 = i3 + a, j1 = i1 + b, j2 = i2 + d;
            if (j3 < 0 || j3 >= G || j1 < 0 || j1 >= G || j2 < 0 || j2 >= G) continue;
            nb += n[(size_t)(j3 * G + j1) * G + j2];
        }
        total += (double)fc * (double)nb;
    }
    return total;
}

// the frame's census: force terms of the own pair pass, particles the force pass visits and live particles (whole system)
struct Census { double terms = 0; int64_t with_force = 0, live = 0; };

// One benchmark run: what it works with, and what it has measured so far
struct Bench {
    Ring &R;
    const Options &o;
    const psamd_sizes &sz;
    int64_t *d_red = nullptr;           // collectives on host numbers: a device scratch word, RCCL, the transfer stream
    Census before, after;
    int settle = 0, period = 1;
    size_t stage_steps = 0;             // timed steps that carried the stage events
    double elapsed = 0, sustained_ms = 0;
    double us[PSAMD_NUM_TIMERS], us_med[PSAMD_NUM_TIMERS], us_max[PSAMD_NUM_TIMERS];
    int64_t launches = 0, own_updates = 0, updates = 0;
    psamd_counters cn{};                // rank 0's (the first local slab's) after the timed region
    std::string clock = "null", sustained_clock = "null";
    std::vector<int64_t> tab;           // [world][7]: build pairs apply finish | wait for halo, force, xfer, in nanoseconds
};

// (a world of one communicator rank -- loopback -- has nothing to reduce)
int reduce_i64(Bench &B, int64_t *host, size_t count, ncclRedOp_t op)
{
    Ring &R = B.R;
    if (R.loopback || R.world == 1) return 0;
    HIP_OK(hipMemcpyAsync(B.d_red, host, count * sizeof(int64_t), hipMemcpyHostToDevice, R.transfer));
    NCCL_OK(ncclAllReduce(B.d_red, B.d_red, count, ncclInt64, op, R.comm, R.transfer));
    HIP_OK(hipMemcpyAsync(host, B.d_red, count * sizeof(int64_t), hipMemcpyDeviceToHost, R.transfer));
    HIP_OK(hipStreamSynchronize(R.transfer));
    return 0;
}

// every rank's device work is done, then all ranks meet, then again nothing is in flight
int barrier(Bench &B)
{
    int64_t one = 1;
    return sync_all(B.R) || reduce_i64(B, &one, 1, ncclSum);
}

// each step = one pass over the same cloud, unless the run evolves
int one_step(Bench &B)
{
    if (!B.o.evolve) for (Slab &s : B.R.local) PS_OK(s.ctx, psamd_snapshot_restore(s.ctx));
    return ring_step(B.R, no_hook);
}

// One step with the counts read back between the stages: particles per cell (whole system) and particles the force pass
// visits per cell (own, and whole system)
int census(Bench &B, Census *out)
{
    Ring &R = B.R;
    const psamd_sizes &sz = B.sz;
    std::vector<int32_t> cellgrid((size_t)sz.n_cellgrid), fc((size_t)sz.num_cells), f_own((size_t)sz.num_cells);
    std::vector<int64_t> n_cell((size_t)sz.num_cells, 0), f_all((size_t)sz.num_cells, 0);
    if (!B.o.evolve) for (Slab &s : R.local) PS_OK(s.ctx, psamd_snapshot_restore(s.ctx));
    const size_t stride = 1 + (size_t)sz.max_per_cell;
    auto hook = [&](int stage) -> int {
        for (Slab &s : R.local) {
            if (stage == 0) {
                PS_OK(s.ctx, psamd_download_cellgrid(s.ctx, cellgrid.data()));
                for (int c = 0; c < sz.num_cells; c++) n_cell[(size_t)c] += cellgrid[stride * (size_t)c];
            } else {
                PS_OK(s.ctx, psamd_download_force_counts(s.ctx, fc.data()));
                if (&s == &R.local[0]) f_own = fc;
                for (int c = 0; c < sz.num_cells; c++) f_all[(size_t)c] += fc[(size_t)c];
            }
        }
        return 0;
    };
    if (ring_step(R, hook)) return 1;
    if (sync_all(R)) return 1;
    if (reduce_i64(B, n_cell.data(), n_cell.size(), ncclSum)) return 1;
    if (reduce_i64(B, f_all.data(), f_all.size(), ncclSum)) return 1;
    *out = Census{force_terms(n_cell, f_own, sz.grid_dim, B.o.all_pairs), 0, 0};
    for (int c = 0; c < sz.num_cells; c++) { out->with_force += f_all[(size_t)c]; out->live += n_cell[(size_t)c]; }
    return 0;
}

// untimed: let the clocks settle, then the warm-up, which runs straight into the timed region
int settle_and_warm(Bench &B)
{
    { psamd_ctx *c = B.R.local[0].ctx; PS_OK(c, psamd_set_timing(c, 1)); PS_OK(c, psamd_set_timing(c, 0)); }      // (the timers' events exist before the timed region)
    // all ranks must take the same number of steps: they decide together, ten at a time
    const auto t_end = std::chrono::steady_clock::now() + std::chrono::duration<double>(B.o.settle_seconds);
    for (;;) {
        int64_t go = (!B.o.evolve && std::chrono::steady_clock::now() < t_end) ? 1 : 0;
        if (reduce_i64(B, &go, 1, ncclMin)) return 1;
        if (!go) break;
        for (int k = 0; k < 10; k++) if (one_step(B)) return 1;
        B.settle += 10;
    }
    for (int k = 0; k < B.o.warmup; k++) if (one_step(B)) return 1;
    return barrier(B);
}

// the particles every local slab has processed so far
int processed(Bench &B, int64_t *sum)
{
    psamd_counters cn{};
    *sum = 0;
    for (Slab &s : B.R.local) { PS_OK(s.ctx, psamd_get_counters(s.ctx, &cn)); *sum += cn.particles_processed; }
    return 0;
}

// the timed steps, with the library's kernel timers and this host's stage events on every period-th of them
int timed_region(Bench &B)
{
    Ring &R = B.R;
    const int steps = B.o.steps;
    psamd_ctx *c0 = R.local[0].ctx;
    B.period = std::max(1, std::min(B.o.timing_period, steps));
    PS_OK(c0, psamd_set_timing_period(c0, B.period));
    PS_OK(c0, psamd_set_timing(c0, 1));
    // this host's own events around the four stage calls of every local slab, on the same steps
    R.stage_ev.assign((size_t)((steps + B.period - 1) / B.period), std::vector<hipEvent_t>(R.local.size() * 8));
    for (auto &v : R.stage_ev) for (auto &e : v) HIP_OK(hipEventCreate(&e));
    int64_t processed0 = 0, processed1 = 0;
    if (processed(B, &processed0)) return 1;
    ClockWatch clock(B.o.device, B.o.clock_ms);
    if (barrier(B)) return 1;
    clock.start();
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < steps; k++) {
        // (the stage events go in on other steps than the library's kernel timers: side by side each delays what the other brackets)
        R.stage_slot = k % B.period == (B.period > 1 ? B.period / 2 : 0) ? k / B.period : -1;
        if (R.stage_slot >= 0) B.stage_steps = (size_t)R.stage_slot + 1;
        if (one_step(B)) return 1;
    }
    R.stage_slot = -1;
    if (barrier(B)) return 1;
    B.elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    clock.end();
    B.clock = clock.json();
    PS_OK(c0, psamd_get_timing(c0, B.us, &B.launches));
    PS_OK(c0, psamd_get_timing_stats(c0, B.us_med, B.us_max, nullptr));
    PS_OK(c0, psamd_set_timing(c0, 0));
    if (processed(B, &processed1)) return 1;
    PS_OK(c0, psamd_get_counters(c0, &B.cn));
    B.own_updates = processed1 - processed0;
    return 0;
}

// a short timed region says little about the clock a long run holds: the same loop again, long enough (no events)
int sustained_region(Bench &B)
{
    const int steps = B.o.sustained_steps;
    ClockWatch clock(B.o.device, B.o.clock_ms);
    if (barrier(B)) return 1;
    clock.start();
    const auto s0 = std::chrono::steady_clock::now();
    for (int k = 0; k < steps; k++) if (one_step(B)) return 1;
    if (barrier(B)) return 1;
    int64_t ns = (int64_t)(1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - s0).count() / steps * 1e6);
    clock.end();
    B.sustained_clock = clock.json();
    if (reduce_i64(B, &ns, 1, ncclMax)) return 1;
    B.sustained_ms = (double)ns * 1e-6;
    return 0;
}

// stage and wait times: the median over the timed steps per local slab, then every rank's figures on every rank
// ([world][7]: build pairs apply finish | wait for halo, force, xfer), in nanoseconds through the int64 all-reduce
// (each rank fills its own rows, the others' are zero: a sum is an all-gather)
int stage_table(Bench &B)
{
    Ring &R = B.R;
    B.tab.assign((size_t)R.world * 7, 0);
    for (size_t i = 0; i < R.local.size(); i++) {
        const int a[7] = {0, 2, 4, 6, 1, 3, 5}, b[7] = {1, 3, 5, 7, 2, 4, 6};
        for (int k = 0; k < 7; k++) {
            std::vector<float> v;
            // (only the steps that recorded them: asking an event that never was recorded for its time fails AND leaves
            // the error behind for the next launch check to find)
            for (size_t q = 0; q < B.stage_steps; q++) {
                const auto &evs = R.stage_ev[q];
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, evs[i * 8 + (size_t)a[k]], evs[i * 8 + (size_t)b[k]]) == hipSuccess) v.push_back(ms);
            }
            std::sort(v.begin(), v.end());
            B.tab[(size_t)R.local[i].rank * 7 + (size_t)k] = v.empty() ? 0 : (int64_t)(1e6 * (double)v[v.size() / 2]);
        }
    }
    if (reduce_i64(B, B.tab.data(), B.tab.size(), ncclSum)) return 1;
    for (auto &v : R.stage_ev) for (auto &e : v) (void)hipEventDestroy(e);
    (void)hipGetLastError();
    return 0;
}

// The record is built so that each key sits beside its value: `"key": value` appended to an object that began as "{".
__attribute__((format(printf, 3, 4))) void put(std::string &obj, const char *key, const char *fmt, ...)
{
    va_list ap, ap2;
    va_start(ap, fmt);
    va_copy(ap2, ap);
    std::string v((size_t)std::vsnprintf(nullptr, 0, fmt, ap), '\0');
    std::vsnprintf(&v[0], v.size() + 1, fmt, ap2);
    va_end(ap);
    va_end(ap2);
    obj += std::string(obj.back() == '{' ? "" : ", ") + "\"" + key + "\": " + v;
}
const char *tf(bool b) { return b ? "true" : "false"; }

std::string timers_json(const Bench &B, const double *v, double div)
{
    static const char *names[PSAMD_NUM_TIMERS] = {"hist", "scan", "scatter", "sort_cells", "pairs", "apply", "lifecycle", "init_iframe", "collide"};
    std::string s = "{";
    for (int k = 0; k < PSAMD_NUM_TIMERS; k++) if (B.us[k] > 0) put(s, names[k], "%.3f", v[k] / div);
    return s + "}";
}

// per-rank stage times, and the waits as minimum / maximum over the ranks
std::string stages_json(const Bench &B, bool waits)
{
    static const char *stage_names[4] = {"build", "pairs", "apply", "finish"}, *wait_names[3] = {"halo", "force", "xfer"};
    const int world = B.R.world;
    std::string s = "{";
    for (int k = 0; k < (waits ? 3 : 4); k++) {
        int64_t lo = INT64_MAX, hi = 0;
        std::string each;
        for (int r = 0; r < world; r++) {
            const int64_t ns = B.tab[(size_t)r * 7 + (waits ? 4 : 0) + (size_t)k];
            char b[32];
            std::snprintf(b, sizeof b, "%s%.4f", r ? ", " : "", (double)ns * 1e-6);
            each += b; lo = std::min(lo, ns); hi = std::max(hi, ns);
        }
        if (waits) put(s, wait_names[k], "{\"min\": %.4f, \"max\": %.4f}", (double)lo * 1e-6, (double)hi * 1e-6);
        else put(s, stage_names[k], "[%s]", each.c_str());
    }
    return s + "}";
}

int print_record(Bench &B)
{
    const Options &o = B.o;
    Ring &R = B.R;
    const psamd_slab_buffers &b = R.local[0].b;
    const bool many = o.world > 1;
    int64_t gl = 0, gc = 0;
    const int grc = psamd_get_graph_stats(R.local[0].ctx, &gl, &gc);
    int rccl_ranks = R.comm ? 0 : 1;
    if (R.comm) NCCL_OK(ncclCommCount(R.comm, &rccl_ranks));
    std::string r = "{", m = "{", p = "{";
    put(r, "psamd_ring", "1"); put(r, "world", "%d", o.world); put(r, "loopback", "%s", tf(o.loopback)); put(r, "rccl_ranks", "%d", rccl_ranks);
    put(r, "n", "%lld", (long long)o.n); put(r, "grid_dim", "%d", B.sz.grid_dim);
    put(r, "steps", "%d", o.steps); put(r, "warmup", "%d", o.warmup); put(r, "settle_steps", "%d", B.settle);
    put(r, "elapsed_s", "%.9f", B.elapsed);
    put(r, "updates", "%lld", (long long)B.updates); put(r, "own_updates", "%lld", (long long)B.own_updates);
    put(r, "live_after", "%lld", (long long)B.after.live); put(r, "particles_with_a_force_term", "%lld", (long long)B.after.with_force);
    put(r, "pairs_rank0", "%.6e", 0.5 * (B.before.terms + B.after.terms));
    put(r, "kernel_us", "%s", timers_json(B, B.us, (double)std::max<int64_t>(B.launches, 1)).c_str());
    put(r, "kernel_us_median", "%s", timers_json(B, B.us_med, 1.0).c_str()); put(r, "kernel_us_max", "%s", timers_json(B, B.us_max, 1.0).c_str());
    put(r, "timed_launches", "%lld", (long long)B.launches); put(r, "timing_period", "%d", B.period);
    put(r, "stage_ms_per_rank", "%s", stages_json(B, false).c_str()); put(r, "wait_ms", "%s", stages_json(B, true).c_str());
    put(r, "relocations", "%lld", (long long)B.cn.relocations); put(r, "relocations_lost", "%lld", (long long)B.cn.relocations_lost);
    put(r, "cell_overflow_kills", "%lld", (long long)B.cn.cell_overflow_kills);
    put(m, "halo_up", "%lld", (long long)b.halo_out_bytes[1]); put(m, "halo_down", "%lld", (long long)b.halo_out_bytes[0]);
    put(m, "force_in", "%lld", (long long)b.force_in_bytes); put(m, "xfer_each", "%lld", (long long)b.xfer_bytes);
    put(m, "status", "%lld", (long long)b.status_bytes); put(m, "snapshot_block", "%lld", (long long)b.allg_bytes);
    put(r, "message_bytes_rank0", "%s}", m.c_str());
    put(p, "halo", "%lld", (long long)(b.halo_out_bytes[0] + b.halo_out_bytes[1])); put(p, "force", "%lld", (long long)b.force_out_bytes);
    put(p, "xfer", "%lld", (long long)(many ? 2 * b.xfer_bytes + 2 * b.xfer2_bytes : 0));
    put(p, "gathers", "%lld", (long long)(many ? b.status_bytes + b.allg_bytes + b.far_bytes : 0));
    put(r, "bytes_per_phase_rank0", "%s}", p.c_str());
    put(r, "rccl_mb_rank0", "%.3f", R.moved / 1e6);
    put(r, "graphs", "%s", tf(o.graphs && grc == PSAMD_OK)); put(r, "graph_replays", "%lld", (long long)gl); put(r, "graph_captures", "%lld", (long long)gc);
    put(r, "side_stream", "%s", tf(o.side_stream != 0)); put(r, "overlap_interior", "%s", tf(o.overlap_interior));
    put(r, "all_pairs", "%s", tf(o.all_pairs)); put(r, "far", "\"%s\"", o.far.empty() ? "none" : o.far.c_str());
    put(r, "force_terms_count", "\"%s\"", o.far.empty() ? "all" : "stencil terms only (the far bodies are not counted)");
    put(r, "fast_math", "%s", tf(o.fast_math)); put(r, "evolve", "%s", tf(o.evolve));
    put(r, "halo_cap_cell", "%d", o.halo_cap_cell); put(r, "xfer_cap", "%d", o.xfer_cap); put(r, "side_stream_mode", "%d", o.side_stream);
    put(r, "shader_clock_mhz", "%s", B.clock.c_str());
    put(r, "sustained_steps", "%d", o.sustained_steps > o.steps ? o.sustained_steps : 0); put(r, "sustained_ms_per_step", "%.6f", B.sustained_ms);
    put(r, "sustained_shader_clock_mhz", "%s", B.sustained_clock.c_str());
    std::printf("%s}\n", r.c_str());
    std::fflush(stdout);
    return 0;
}

int run_bench(Ring &R, const Options &o, const psamd_sizes &sz)
{
    Bench B{R, o, sz};
    HIP_OK(hipMalloc((void **)&B.d_red, ((size_t)sz.num_cells + 8) * sizeof(int64_t)));
    if (!o.evolve) for (Slab &s : R.local) PS_OK(s.ctx, psamd_snapshot_save(s.ctx));
    // (The census -- downloads, host work -- comes BEFORE the settling steps and the warmup, so that the warmup runs
    // straight into the timed region: an idle GPU in between cost the first timed steps their clock.)
    if (!o.evolve && census(B, &B.before)) return bail();
    if (settle_and_warm(B) || timed_region(B)) return bail();
    if (o.sustained_steps > o.steps && !o.evolve && sustained_region(B)) return bail();
    if (stage_table(B) || census(B, &B.after)) return bail();
    if (o.evolve) B.before = B.after;
    int64_t ns = (int64_t)(B.elapsed * 1e9);
    B.updates = B.own_updates;
    if (reduce_i64(B, &B.updates, 1, ncclSum) || reduce_i64(B, &ns, 1, ncclMax)) return bail();
    B.elapsed = (double)ns * 1e-9;
    if ((o.rank == 0 || o.loopback) && print_record(B)) return bail();
    if (barrier(B)) return bail();
    (void)hipFree(B.d_red);
    return 0;
}

}  // namespace
