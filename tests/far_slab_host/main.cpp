// The HIP-free host code of the far field on slabs, as a stand-alone program (tests/test_far_slab_cpu.py builds it with the
// host sanitizers and runs it once): the ring host's command line (host/ring_options.hpp), the slab plans of every rank
// (partition.hpp) and the size of the all-gathered block of cell sums -- what create.hip derives a far slab's message from.
//   far_slab_host [ring options] [--cuts c0,c1,...]      prints: far model, planes, allg_cells, block bytes, then (first cell, cells) by rank
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../host/ring_options.hpp"
#include "../../particlesystem_amd/csrc/geometry.hpp"
#include "../../particlesystem_amd/csrc/partition.hpp"

int main(int argc, char **argv)
{
    std::vector<int> cuts;
    std::vector<char *> rest;
    for (int i = 0; i < argc; i++) {
        if (std::string(argv[i]) == "--cuts" && i + 1 < argc) {
            for (const char *p = argv[++i]; *p;) { cuts.push_back(std::atoi(p)); while (*p && *p != ',') p++; if (*p) p++; }
        } else rest.push_back(argv[i]);
    }
    Options o;
    if (const int rc = parse_args((int)rest.size(), rest.data(), o)) return rc;
    psamd_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.max_particles_num = 16384; cfg.x_factor = 2; cfg.chunk_factor = o.chunk_factor; cfg.chunk_dim = o.chunk_dim;
    cfg.cell_size = 5.0; cfg.dt = 0.05; cfg.life_steps = 300.0;
    psamd::Geometry g;
    if (!g.init(cfg)) { std::fprintf(stderr, "bad grid\n"); return 2; }
    if (!cuts.empty() && (int)cuts.size() != o.world + 1) { std::fprintf(stderr, "--cuts takes world + 1 numbers\n"); return 2; }
    std::vector<int> first, cells;
    const int most = psamd::gather_block_cells(g.F, g.D, g.seg_base, g.seg_size_t, g.info_base, o.world, cuts.empty() ? nullptr : cuts.data(), &first, &cells);
    if (!most) { std::fprintf(stderr, "no slab partition for this grid and world size\n"); return 1; }
    const int planes = far_model(o) == 3 ? 10 : 4;
    std::printf("%d %d %d %zu\n", far_model(o), planes, most, psamd::far_slab_block_bytes(planes, most));
    for (int r = 0; r < o.world; r++) std::printf("%d %d\n", first[(size_t)r], cells[(size_t)r]);
    return 0;
}
