// ring_options.hpp -- the command line of ps_ring_rccl (part of ps_ring_rccl.cpp, which alone includes it).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace {

struct Options {
    int world = 2, rank = 0, iters = 8, device = -1;
    int64_t n = 60000, max_particles = 0;
    uint32_t seed = 2026;
    uint64_t job = 0;
    std::string id_file;
    std::string far;                                                 // "", or the far-field force model: flat, pyramid, quadrupole
    bool loopback = false, all_pairs = false, births = false, graphs = false, bench = false, evolve = false, overlap_interior = false, fast_math = false;
    bool id_only = false, launch_check = false, routes = false;     // the hooks that need no GPU
    bool break_sizes = false;                                        // (test hook: rank 1 is created with other message sizes than its neighbours expect)
    int side_stream = 0, wait_policy = -1;
    int steps = 200, warmup = 5, timing_period = 8, sustained_steps = 0;
    int clock_ms = 10;                                               // how often the shader clock is sampled while a timed region runs (0: not at all)
    double settle_seconds = 0.5;
    int chunk_factor = 4, chunk_dim = 4, halo_cap_cell = 0, xfer_cap = 0;
};

const struct { const char *name; bool Options::*flag; } kFlags[] = {
    {"--loopback", &Options::loopback}, {"--id-only", &Options::id_only}, {"--launch-check", &Options::launch_check}, {"--routes", &Options::routes},
    {"--test-size-mismatch", &Options::break_sizes}, {"--all-pairs", &Options::all_pairs}, {"--births", &Options::births}, {"--fast-math", &Options::fast_math},
    {"--overlap-interior", &Options::overlap_interior}, {"--bench", &Options::bench}, {"--evolve", &Options::evolve}};
const struct { const char *name; int Options::*value; } kInts[] = {
    {"--world", &Options::world}, {"--rank", &Options::rank}, {"--device", &Options::device}, {"--iters", &Options::iters}, {"--wait", &Options::wait_policy},
    {"--steps", &Options::steps}, {"--warmup", &Options::warmup}, {"--clock-period-ms", &Options::clock_ms}, {"--chunk-factor", &Options::chunk_factor},
    {"--chunk-dim", &Options::chunk_dim}, {"--halo-cap-cell", &Options::halo_cap_cell}, {"--xfer-cap", &Options::xfer_cap},
    {"--side-stream", &Options::side_stream}, {"--timing-period", &Options::timing_period}, {"--sustained-steps", &Options::sustained_steps}};

// the far-field model of --far as a number: 0 none, 1 flat, 2 pyramid, 3 pyramid with quadrupoles (ps_ring_rccl.cpp turns it
// into the context's flags; this header knows nothing of the library)
inline int far_model(const Options &o) { return o.far == "flat" ? 1 : o.far == "pyramid" ? 2 : o.far == "quadrupole" ? 3 : 0; }

// 0, or the exit status (2: an unknown option, or options that do not make a run)
int parse_args(int argc, char **argv, Options &o)
{
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char * { return i + 1 < argc ? argv[++i] : "0"; };
        bool known = false;
        for (const auto &f : kFlags) if (a == f.name) { o.*f.flag = true; known = true; }
        for (const auto &v : kInts) if (a == v.name) { o.*v.value = std::atoi(next()); known = true; }
        if (known) continue;
        if (a == "--n") o.n = std::atoll(next());
        else if (a == "--max-particles") o.max_particles = std::atoll(next());
        else if (a == "--seed") o.seed = (uint32_t)std::atoll(next());
        else if (a == "--id-file") o.id_file = next();
        else if (a == "--far") {
            o.far = i + 1 < argc ? argv[++i] : "";
            if (!far_model(o)) { std::fprintf(stderr, "--far takes flat, pyramid or quadrupole\n"); return 2; }
        }
        else if (a == "--job") o.job = (uint64_t)std::strtoull(next(), nullptr, 10);
        else if (a == "--graphs") o.graphs = std::atoi(next()) != 0;
        else if (a == "--settle-seconds") o.settle_seconds = std::atof(next());
        else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    if (!o.far.empty() && o.all_pairs) {
        std::fprintf(stderr, "--far and --all-pairs are two force models: choose one\n");
        return 2;
    }
    o.side_stream = std::max(0, std::min(2, o.side_stream));
    o.timing_period = std::max(1, o.timing_period);
    o.sustained_steps = std::max(0, o.sustained_steps);
    if (o.world < 1 || o.rank < 0 || o.rank >= o.world || (!o.routes && !o.loopback && o.world > 1 && o.id_file.empty())) {
        std::fprintf(stderr, "usage: ps_ring_rccl --world W (--loopback | --rank r --id-file F --job J [--device d]) [--n N] [--iters K] [--seed S] "
                             "[--all-pairs | --far flat|pyramid|quadrupole] [--births] [--graphs 0|1] [--side-stream 0|1|2] [--overlap-interior] [--bench --steps K --warmup W ...]\n");
        return 2;
    }
    if (o.device < 0) o.device = o.loopback ? 0 : o.rank;
    return 0;
}

}  // namespace
