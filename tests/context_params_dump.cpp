// context_params_dump.cpp -- what context creation derives before it touches the device (csrc/context_params.hpp), for
// configurations read from standard input: the stand-alone program of tests/test_context_params_cpu.py.  One configuration
// per line, every number of psamd_config in this order (doubles in decimal, as many digits as it takes):
//   max_particles_num x_factor chunk_factor chunk_dim cell_size eps2 collision_radius particle_weight dt max_v
//   explosion_speed life_steps flags seed rank world halo_cap_cell xfer_cap xfer_cap_max drag force_sign one_pass
//   <number of cuts> <cuts ...>
// For each the program prints "status <n>", "why <text>" and -- where the status is 0 -- one line "<field> <values ...>" per
// field of ContextParams (floats and doubles as their bits, 0x...), then "end".
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "context_params.hpp"

using namespace psamd;

static void ints(const char *name, const int32_t *v, int n)
{
    std::printf("%s", name);
    for (int k = 0; k < n; k++) std::printf(" %d", v[k]);
    std::printf("\n");
}
static void one(const char *name, long long v) { std::printf("%s %lld\n", name, v); }
static void f32(const char *name, float f) { uint32_t u; std::memcpy(&u, &f, 4); std::printf("%s 0x%08" PRIx32 "\n", name, u); }
static void f64(const char *name, double f) { uint64_t u; std::memcpy(&u, &f, 8); std::printf("%s 0x%016" PRIx64 "\n", name, u); }

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        psamd_config c{};
        int one_pass = 0, ncuts = 0;
        in >> c.max_particles_num >> c.x_factor >> c.chunk_factor >> c.chunk_dim >> c.cell_size >> c.eps2 >> c.collision_radius
           >> c.particle_weight >> c.dt >> c.max_v >> c.explosion_speed >> c.life_steps >> c.flags >> c.seed >> c.rank >> c.world
           >> c.halo_cap_cell >> c.xfer_cap >> c.xfer_cap_max >> c.drag >> c.force_sign >> one_pass >> ncuts;
        for (int k = 0; k < ncuts && k <= PSAMD_MAX_RANKS; k++) in >> c.cuts[k];
        if (!in) { std::printf("status -1\nwhy unreadable line\nend\n"); continue; }
        Geometry g;
        if (!g.init(c)) { std::printf("status -2\nwhy geometry\nend\n"); continue; }
        ContextParams o;
        std::string why;
        const int status = derive_context_params(c, g, one_pass != 0, o, why);
        std::printf("status %d\nwhy %s\n", status, why.c_str());
        if (status != PSAMD_OK) { std::printf("end\n"); continue; }
        const SlabPlan &p = o.plan;
        const int32_t plan[] = {p.world, p.rank, p.G, p.D, p.F, p.cut_lo, p.cut_hi, p.state_lo, p.state_hi, p.group_lo, p.group_hi, p.below_lo, p.below_hi,
                                p.above_lo, p.above_hi, p.lentin_lo, p.lentin_hi, p.lentout_lo, p.lentout_hi, p.send_up_lo, p.send_up_hi,
                                p.send_down_lo, p.send_down_hi, p.up_rank, p.down_rank, p.valid ? 1 : 0};
        ints("plan", plan, (int)(sizeof plan / sizeof plan[0]));
        ints("plan.slot_lo", p.slot_lo, 4); ints("plan.slot_hi", p.slot_hi, 4);
        ints("plan.rec_lo", p.rec_lo, 4); ints("plan.rec_hi", p.rec_hi, 4);
        const DevParams &P = o.P;
        one("P.G", P.G); one("P.num_cells", P.num_cells); one("P.num_chunks", P.num_chunks); one("P.container", P.container);
        one("P.max_per_cell", P.max_per_cell); one("P.max_per_chunk", P.max_per_chunk); one("P.slices", P.slices); one("P.flags", P.flags);
        f32("P.t", P.t); f32("P.kid_thr", P.kid_thr); f32("P.life_thr", P.life_thr); f32("P.coll_d2_gate", P.coll_d2_gate);
        f32("P.dmax", P.dmax); f32("P.vmax", P.vmax); f32("P.w_default", P.w_default); f32("P.fert_lo", P.fert_lo); f32("P.fert_hi", P.fert_hi);
        f64("P.cell_size", P.cell_size); f64("P.eps2", P.eps2); f64("P.coll_radius", P.coll_radius); f64("P.kid_age", P.kid_age);
        f64("P.life", P.life); f64("P.expl_speed", P.expl_speed);
        std::printf("P.seed %" PRIu64 "\n", P.seed);
        one("P.key_chunk_shift", P.key_chunk_shift); one("P.key_rec_shift", P.key_rec_shift); one("P.key_bits", P.key_bits);
        one("P.lean_math", P.lean_math); f32("P.eps2f", P.eps2f); f32("P.eps_f32_from", P.eps_f32_from); f32("P.slow_below", P.slow_below);
        f32("P.halo_reach", P.halo_reach); f32("P.coll_d2_max", P.coll_d2_max); one("P.two_pass", P.two_pass); f32("P.pad_f", P.pad_f);
        ints("P.reg_first", P.reg_first, 4); ints("P.reg_layers", P.reg_layers, 4); ints("P.reg_base", P.reg_base, 4); ints("P.reg_sorted", P.reg_sorted, 4);
        one("P.n_local_cells", P.n_local_cells); one("P.n_own_cells", P.n_own_cells); one("P.sorted_cap", P.sorted_cap);
        one("P.own_comp0", P.own_comp0); one("P.own_comp1", P.own_comp1);
        ints("P.comp_lo", P.comp_lo, 3); ints("P.comp_hi", P.comp_hi, 3);
        ints("P.slot_lo", P.slot_lo, 4); ints("P.slot_n", P.slot_n, 4); one("P.slots_total", P.slots_total);
        ints("P.rec_lo", P.rec_lo, 4); ints("P.rec_hi", P.rec_hi, 4);
        one("P.rank", P.rank); one("P.world", P.world); one("P.halo_cap_cell", P.halo_cap_cell);
        one("P.xfer_cap", P.xfer_cap); one("P.xfer_cap_max", P.xfer_cap_max); one("P.xfer_cap0", P.xfer_cap0);
        one("P.lentout_c0", P.lentout_c0); one("P.lentout_c1", P.lentout_c1); one("P.num_cells_global", P.num_cells_global);
        f32("P.drag", P.drag); f32("P.force_sign", P.force_sign);
        one("P.allg_cells", P.allg_cells); one("P.allg_cap", P.allg_cap); one("P.allg_block", P.allg_block); one("P.status_words", P.status_words);
        ints("P.nbr_rec_lo", &P.nbr_rec_lo[0][0], 8); ints("P.nbr_rec_hi", &P.nbr_rec_hi[0][0], 8);
        one("P.xfer2_cap", P.xfer2_cap); one("P.far_cap", P.far_cap);
        ints("S.seg_base", o.S.seg_base, 5); ints("S.info_base", o.S.info_base, 5); ints("S.seg_size_t", o.S.seg_size_t, 4);
        one("have_interior", o.have_interior);
        ints("int_lo", o.int_lo, 3); ints("int_hi", o.int_hi, 3); ints("rest_lo", o.rest_lo, 3); ints("rest_hi", o.rest_hi, 3);
        one("ops_cap", o.ops_cap); one("moves_cap", o.moves_cap); one("frame_ints", (long long)o.frame_ints); one("xfer_room", (long long)o.xfer_room);
        ints("halo_out_c0", o.halo_out_c0, 2); ints("halo_out_cells", o.halo_out_cells, 2); ints("halo_in_cells", o.halo_in_cells, 2);
        for (int w = 0; w < MSG_COUNT; w++) std::printf("msg.%d %zu %zu\n", w, o.msg[w].bytes, o.msg[w].alloc);
        one("lev.n", o.lev.n); ints("lev.G", o.lev.G, FAR_MAX_LEVELS); ints("lev.off", o.lev.off, FAR_MAX_LEVELS + 1);
        ints("far_plan", o.far_plan.data(), (int)o.far_plan.size());
        std::printf("end\n");
    }
    return 0;
}
