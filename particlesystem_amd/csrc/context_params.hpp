// context_params.hpp -- everything psamd_create derives before it touches the device: the kernels' parameters, the sizes
// of the step's arrays and of the slab messages, and the refusals, from the configuration, the geometry and the ranks'
// plans.  Host arithmetic only, free of HIP (tests/context_params_dump.cpp runs it without a GPU); create.hip is the
// order of the HIP calls that follow.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/psamd.h"
#include "device_types.h"
#include "geometry.hpp"
#include "partition.hpp"

namespace psamd {

// A slab message (device), by the ABI's `which` numbering (psamd_slab_msg_download in include/psamd.h); in a pair,
// + 0 = the rank below, + 1 = the rank above.  The *_IN of status, allg and far hold every rank's message, all-gathered.
enum { MSG_HALO_OUT = 0, MSG_HALO_IN = 2, MSG_FORCE_OUT = 4, MSG_FORCE_IN, MSG_XFER_OUT = 6, MSG_XFER_IN = 8, MSG_STATUS_OUT = 10, MSG_STATUS_IN,
       MSG_ALLG_OUT, MSG_ALLG_IN, MSG_XFER2_OUT = 14, MSG_XFER2_IN = 16, MSG_FAR_OUT = 18, MSG_FAR_IN, MSG_COUNT };
// the order their buffers are allocated in (create.hip: the sequence of the allocations is load-bearing)
constexpr int MSG_ALLOC_ORDER[MSG_COUNT] = {MSG_HALO_OUT, MSG_HALO_IN, MSG_HALO_OUT + 1, MSG_HALO_IN + 1, MSG_FORCE_OUT, MSG_FORCE_IN,
                                            MSG_XFER_OUT, MSG_XFER_IN, MSG_XFER_OUT + 1, MSG_XFER_IN + 1, MSG_XFER2_OUT, MSG_XFER2_IN,
                                            MSG_XFER2_OUT + 1, MSG_XFER2_IN + 1, MSG_FAR_OUT, MSG_FAR_IN, MSG_ALLG_OUT, MSG_ALLG_IN,
                                            MSG_STATUS_OUT, MSG_STATUS_IN};
// bytes of a transfer message with room for `recs` records
inline size_t xfer_msg_bytes(size_t recs) { return ((size_t)MSG_HEADER_WORDS + recs * (sizeof(XferRec) / sizeof(int))) * sizeof(int); }

// what the far-field flags make of a context: far monopoles (flat or as a pyramid); one whose host has said that it
// all-gathers the cell sums (PSAMD_FLAG_FAR_SLAB); the fp64 planes per cell
inline bool far_context(uint32_t flags) { return (flags & (PSAMD_FLAG_FAR_MONOPOLE | PSAMD_FLAG_FAR_PYRAMID)) != 0; }
inline bool far_slab(uint32_t flags) { return (flags & PSAMD_FLAG_FAR_SLAB) && far_context(flags); }
inline int far_planes(uint32_t flags) { return (flags & PSAMD_FLAG_FAR_QUADRUPOLE) ? 10 : 4; }

struct MsgSize { size_t bytes = 0, alloc = 0; };   // what travels at first; the buffer's room.  0 / 0: the context has no such message

struct ContextParams {
    SlabPlan plan;                    // this rank's
    DevParams P{};                    // every field but eps_f32_from (INFINITY here) and slow_below: the device probe settles them
    SegLayout S{};
    // the pair stage cut in two: interior own cells (no halo needed), the rest; without an interior both are P's ranges
    bool have_interior = false;
    int32_t int_lo[3] = {0, 0, 0}, int_hi[3] = {0, 0, 0}, rest_lo[3] = {0, 0, 0}, rest_hi[3] = {0, 0, 0};
    int ops_cap = 0, moves_cap = 0;
    size_t frame_ints = 0;            // ints zeroed by init_iframe
    size_t xfer_room = 0;             // room of a neighbour transfer message, in records: the most a step can ask for
    int halo_out_c0[2] = {0, 0}, halo_out_cells[2] = {0, 0}, halo_in_cells[2] = {0, 0};
    MsgSize msg[MSG_COUNT];
    FarLevels lev;                    // far contexts: the levels of the moment planes
    std::vector<int> far_plan;        // a far slab: (first global cell, cells) of every rank's state layers, by rank
};

inline bool rank_in_world(const psamd_config &cfg) { return cfg.world >= 1 && cfg.world <= PSAMD_MAX_RANKS && cfg.rank >= 0 && cfg.rank < cfg.world; }

inline SlabPlan plan_for(const Geometry &g, const psamd_config &cfg)
{
    const bool given = cfg.world >= 1 && cfg.world <= PSAMD_MAX_RANKS && cfg.cuts[cfg.world] != 0;
    return make_slab_plan(g.F, g.D, g.seg_base, g.seg_size_t, g.info_base, cfg.rank, cfg.world, given ? cfg.cuts : nullptr);
}

// The rank's place and plan: what psamd_create and psamd_slab_plan_describe refuse before anything else.
inline int rank_plan(const psamd_config &cfg, const Geometry &g, SlabPlan &plan, std::string &why)
{
    if (!rank_in_world(cfg)) { why = "rank/world"; return PSAMD_ERR_INVALID_ARG; }
    plan = plan_for(g, cfg);
    if (plan.valid) return PSAMD_OK;
    why = "no slab partition for this grid and world size (every rank needs >= 2 cell layers "
          "and its neighbours must hold every layer it reads)";
    return PSAMD_ERR_UNSUPPORTED;
}

// DevParams fields that describe what this rank holds (partition.hpp -> device_types.h)
inline void fill_slab_params(const Geometry &g, const SlabPlan &pl, const psamd_config &cfg, DevParams &P)
{
    const int GG = g.G * g.G;
    P.rank = pl.rank; P.world = pl.world; P.num_cells_global = g.num_cells;
    const int first[4] = {pl.state_lo, pl.below_lo, pl.lentin_lo, pl.above_lo};
    const int layers[4] = {pl.state_hi - pl.state_lo, pl.lentin_lo - pl.below_lo, pl.lentin_hi - pl.lentin_lo, pl.above_hi - pl.above_lo};
    P.halo_cap_cell = (cfg.halo_cap_cell > 0 && cfg.halo_cap_cell < g.max_per_cell) ? cfg.halo_cap_cell : g.max_per_cell;
    P.xfer_cap = pl.world > 1 ? (cfg.xfer_cap > 0 ? cfg.xfer_cap : std::max(4096, GG * g.max_per_cell / 4)) : 0;
    // how far the transfer messages may grow (their buffers' room): by default a step's worst case -- everything two cell
    // layers hold, and a child of each (a particle moves one layer a step, two when the rounded sum lands on the far face)
    P.xfer_cap0 = P.xfer_cap;
    P.xfer_cap_max = pl.world > 1 ? std::max(P.xfer_cap, cfg.xfer_cap_max > 0 ? cfg.xfer_cap_max
                                                         : (int)std::min<int64_t>(4ll * GG * g.max_per_cell, INT32_MAX / 256)) : 0;
    int64_t slots = 0;
    for (int t = 0; t < 4; t++) { P.slot_lo[t] = pl.slot_lo[t]; P.slot_n[t] = pl.slot_hi[t] - pl.slot_lo[t]; slots += P.slot_n[t];
                                  P.rec_lo[t] = pl.rec_lo[t]; P.rec_hi[t] = pl.rec_hi[t]; }
    P.slots_total = (int)slots;
    int base = 0;
    int64_t sorted = 0;
    for (int r = 0; r < 4; r++) {
        P.reg_first[r] = first[r]; P.reg_layers[r] = layers[r]; P.reg_base[r] = base; P.reg_sorted[r] = (int)sorted;
        base += layers[r] * GG + 1;                                     // + the gap cell
        // the own block can hold every owned slot (overflow-killed entries keep their place in
        // the sorted order for the frame); a remote block what its messages can carry
        sorted += r == 0 ? slots : (int64_t)layers[r] * GG * P.halo_cap_cell;
    }
    P.n_local_cells = base; P.n_own_cells = layers[0] * GG;
    P.sorted_cap = (int)sorted;
    P.own_comp0 = (std::max(pl.cut_lo, pl.state_lo) - pl.state_lo) * GG;
    P.own_comp1 = (std::min(pl.cut_hi, pl.state_hi) - pl.state_lo) * GG;
    if (P.own_comp1 < P.own_comp0) P.own_comp1 = P.own_comp0;
    // the whole pair stage in one pass: the lent cells, then the own ones
    P.comp_lo[0] = P.reg_base[2]; P.comp_hi[0] = P.reg_base[2] + layers[2] * GG;
    P.comp_lo[1] = P.own_comp0; P.comp_hi[1] = P.own_comp1;
    P.comp_lo[2] = P.comp_hi[2] = 0;
    P.lentout_c0 = (pl.lentout_lo - pl.state_lo) * GG; P.lentout_c1 = (pl.lentout_hi - pl.state_lo) * GG;
}

// the largest squared distance two in-box particles can have, with slack for one wrap of drift
inline double max_d2(const Geometry &g) { const double L = (double)g.G * g.cfg.cell_size; return 3.0 * (2.0 * L) * (2.0 * L); }

// Interior own cells: computed layers whose neighbour layers are both own state (or outside
// the grid): their collision flags and forces need nothing from another rank, so that
// pass can run while the halo messages travel (two-pass mode; slab_pairs_interior).
inline void split_interior(const Geometry &g, ContextParams &o)
{
    const DevParams &P = o.P; const SlabPlan &pl = o.plan;
    const int GG = g.G * g.G, lo = std::max(pl.cut_lo, pl.state_lo), hi = std::min(pl.cut_hi, pl.state_hi);
    auto own = [&](int l) { return l < 0 || l >= g.G || (l >= pl.state_lo && l < pl.state_hi); };
    int i0 = lo, i1 = lo;
    for (int l = lo; l < hi; l++) if (own(l - 1) && own(l + 1)) { if (i1 == i0) i0 = l; i1 = l + 1; } else if (i1 > i0) break;
    for (int k = 0; k < 3; k++) { o.int_lo[k] = o.rest_lo[k] = P.comp_lo[k]; o.int_hi[k] = o.rest_hi[k] = P.comp_hi[k]; }
    o.have_interior = P.world > 1 && P.two_pass && P.lean_math && i1 > i0 && (i1 - i0) < (hi - lo) + (pl.lentin_hi - pl.lentin_lo)
                      && !(P.flags & (PSAMD_FLAG_ALL_PAIRS | PSAMD_FLAG_FAR_MONOPOLE | PSAMD_FLAG_FAR_PYRAMID));
    // (an all-pairs pass needs the gathered snapshot, a far pass the gathered cell sums: nothing to do before they land)
    if (o.have_interior) {
        const int a = (i0 - pl.state_lo) * GG, b = (i1 - pl.state_lo) * GG;
        o.int_lo[0] = a; o.int_hi[0] = b;
        o.int_lo[1] = o.int_hi[1] = o.int_lo[2] = o.int_hi[2] = 0;
        o.rest_lo[1] = P.own_comp0; o.rest_hi[1] = a;
        o.rest_lo[2] = b; o.rest_hi[2] = P.own_comp1;
    }
}

// The sizes of the step's arrays and of the slab messages (see slab.hip "slab exchange"): fixed by the plan.
inline void size_arrays_and_msgs(const Geometry &g, ContextParams &o)
{
    const DevParams &P = o.P; const SlabPlan &pl = o.plan;
    const size_t C = (size_t)P.slots_total, LC = (size_t)P.n_local_cells;
    const size_t xf = o.xfer_room = (size_t)P.xfer_cap_max + (size_t)P.xfer2_cap + (size_t)P.far_cap * (size_t)std::max(1, P.world) / 2 + 1;
    o.ops_cap = (int)std::min<size_t>(3 * C + 2 * xf + 64 + (P.world > 1 ? (size_t)P.world * STATUS_KILL_CAP : 0), (size_t)INT32_MAX / 2);
    o.moves_cap = (int)std::min<size_t>(2 * C + 2 * xf + 64, (size_t)INT32_MAX / 2);
    // cell counts, chunk counts, queue-op counts and cursors per record, halo counts, active-list lengths, hand-off flags of the force pass
    o.frame_ints = LC + g.num_chunks + 2 * (size_t)g.queue_infos + LC + LC + 2 * LC * P.slices;   // (flags: one block per pass of the pair stage)
    if (P.world <= 1) return;
    const int GG = g.G * g.G;
    auto set = [&](int which, size_t bytes, size_t alloc = 0) { o.msg[which] = {bytes, alloc ? alloc : bytes}; };
    auto halo_bytes = [&](int cells) { return ((size_t)MSG_HEADER_WORDS + (size_t)cells + 6 * (size_t)cells * P.halo_cap_cell) * sizeof(int); };
    // out: own layers for the rank below / above; in: what they hold for this rank
    o.halo_out_cells[0] = (pl.send_down_hi - pl.send_down_lo) * GG; o.halo_out_c0[0] = (pl.send_down_lo - pl.state_lo) * GG;
    o.halo_out_cells[1] = (pl.send_up_hi - pl.send_up_lo) * GG;     o.halo_out_c0[1] = (pl.send_up_lo - pl.state_lo) * GG;
    o.halo_in_cells[0] = (pl.below_hi - pl.below_lo) * GG;
    o.halo_in_cells[1] = (pl.above_hi - pl.above_lo) * GG;
    for (int k = 0; k < 2; k++) {
        if (o.halo_out_cells[k] > 0) set(MSG_HALO_OUT + k, halo_bytes(o.halo_out_cells[k]));
        if (o.halo_in_cells[k] > 0) set(MSG_HALO_IN + k, halo_bytes(o.halo_in_cells[k]));
    }
    auto force_bytes = [&](int cells) { return ((size_t)MSG_HEADER_WORDS + 4 * (size_t)cells * P.halo_cap_cell) * sizeof(int); };
    if (P.reg_layers[2] > 0) set(MSG_FORCE_OUT, force_bytes(P.reg_layers[2] * GG));
    if (P.lentout_c1 > P.lentout_c0) set(MSG_FORCE_IN, force_bytes(P.lentout_c1 - P.lentout_c0));
    // to the neighbours (what travels follows P.xfer_cap, psamd_slab_build; room for a step's worst case), then two ranks away
    for (int k = 0; k < 2; k++) {
        set(MSG_XFER_OUT + k, xfer_msg_bytes((size_t)P.xfer_cap + 1), xfer_msg_bytes(xf));
        set(MSG_XFER_IN + k, xfer_msg_bytes((size_t)P.xfer_cap + 1), xfer_msg_bytes(xf));
    }
    for (int k = 0; k < 2 && P.xfer2_cap > 0; k++) {
        set(MSG_XFER2_OUT + k, xfer_msg_bytes((size_t)P.xfer2_cap));
        set(MSG_XFER2_IN + k, xfer_msg_bytes((size_t)P.xfer2_cap));
    }
    if (P.far_cap > 0) {
        set(MSG_FAR_OUT, xfer_msg_bytes((size_t)P.far_cap));
        set(MSG_FAR_IN, xfer_msg_bytes((size_t)P.far_cap) * (size_t)P.world);
    }
    // the all-gathered snapshot, or a far slab's cell sums of every rank's own cells (slab.hip, "far field on slabs"): the
    // all-pairs slot, which a far context leaves free
    const size_t block = (size_t)P.allg_block * sizeof(int);
    if ((P.flags & PSAMD_FLAG_ALL_PAIRS) || far_slab(P.flags)) set(MSG_ALLG_OUT, block);
    if (P.flags & PSAMD_FLAG_ALL_PAIRS) set(MSG_ALLG_IN, block * P.world, block * P.world + 64 * sizeof(int));      // + slack: scalar loads fetch whole groups
    else if (far_slab(P.flags)) set(MSG_ALLG_IN, block * P.world);
    set(MSG_STATUS_OUT, (size_t)P.status_words * sizeof(int));
    set(MSG_STATUS_IN, (size_t)P.status_words * sizeof(int) * P.world);
}

// Everything the kernels' parameters (o.P, o.S) and the sizes take from the configuration, the geometry and the ranks'
// plans; the PSAMD_* status, and on a refusal why.  one_pass: PSAMD_ONE_PASS is set.
inline int derive_context_params(const psamd_config &cfg, const Geometry &g, bool one_pass, ContextParams &o, std::string &why)
{
    auto refuse = [&](int status, const std::string &what) { why = what; return status; };
    o = ContextParams();
    if (const int rc = rank_plan(cfg, g, o.plan, why)) return rc;
    DevParams &P = o.P;
    P.G = g.G; P.num_cells = g.num_cells; P.num_chunks = g.num_chunks; P.container = g.container;
    P.max_per_cell = g.max_per_cell; P.max_per_chunk = g.max_per_chunk;
    P.slices = (g.max_per_cell + 63) / 64;
    P.flags = cfg.flags;
    P.t = (float)cfg.dt;
    P.kid_thr = float_ceil(g.kid_age);
    P.life_thr = float_floor(g.particle_life);
    // every pair whose fp32 squared distance is at or below this gets the exact
    // collision test; the margin only has to cover the rounding of sqrtf
    P.coll_d2_gate = (float)(cfg.collision_radius * cfg.collision_radius * 1.001 + 1e-30);
    P.dmax = (float)cfg.cell_size;   // MAX_DX = CELL_SIZE, common.h:65
    P.vmax = (float)cfg.max_v;
    P.w_default = (float)cfg.particle_weight;
    P.fert_lo = (float)g.min_fert; P.fert_hi = (float)g.max_fert;
    P.cell_size = cfg.cell_size; P.eps2 = cfg.eps2; P.coll_radius = cfg.collision_radius;
    P.kid_age = g.kid_age; P.life = g.particle_life; P.expl_speed = cfg.explosion_speed;
    P.seed = cfg.seed;
    P.drag = (float)cfg.drag;
    P.force_sign = cfg.force_sign < 0 ? -1.0f : 1.0f;
    if (cfg.drag < 0) return refuse(PSAMD_ERR_INVALID_ARG, "drag must be >= 0");
    if ((cfg.flags & PSAMD_FLAG_FAR_SLAB) && !(cfg.flags & (PSAMD_FLAG_FAR_MONOPOLE | PSAMD_FLAG_FAR_PYRAMID)))
        return refuse(PSAMD_ERR_INVALID_ARG, "PSAMD_FLAG_FAR_SLAB is a modifier of PSAMD_FLAG_FAR_MONOPOLE and PSAMD_FLAG_FAR_PYRAMID: set one of them too");
    fill_slab_params(g, o.plan, cfg, P);
    P.status_words = STATUS_CHUNK_OFF + 4 * g.num_chunks;
    if (cfg.world > 1) {
        // the ring neighbours' queue records; and whether any rank's whole state is ONE cell layer: a particle
        // that crosses two layers in a step (from one ulp below a face, moved by exactly CELL_SIZE) can fly over
        // such a rank, to the rank beyond it -- those records get outboxes of their own, sent straight to rank +-2.
        // All-pairs: every rank's block of the all-gathered snapshot has the same size, room for the rank with the
        // most cells / slots.  A far slab (PSAMD_FLAG_FAR_SLAB): its block of the all-gathered cell sums likewise, room for the
        // rank with the most cells -- and what every rank's block must say of itself: (first global cell, cells) by rank.
        bool single = false;
        int cells = 0;
        int64_t slots = 0;
        psamd_config rc = cfg;
        for (int r = 0; r < cfg.world; r++) {
            rc.rank = r;
            const SlabPlan pr = plan_for(g, rc);
            if (!pr.valid) return refuse(PSAMD_ERR_UNSUPPORTED, "no slab partition for this grid and world size");
            single |= pr.state_hi - pr.state_lo < 2;
            const int which = r == (cfg.rank + cfg.world - 1) % cfg.world ? 0 : -1, which2 = r == (cfg.rank + 1) % cfg.world ? 1 : -1;
            for (int w : {which, which2})
                if (w >= 0) for (int t = 0; t < 4; t++) { P.nbr_rec_lo[w][t] = pr.rec_lo[t]; P.nbr_rec_hi[w][t] = pr.rec_hi[t]; }
            int64_t sl = 0;
            for (int t = 0; t < 4; t++) sl += pr.slot_hi[t] - pr.slot_lo[t];
            const int n = (pr.state_hi - pr.state_lo) * g.G * g.G;
            cells = std::max(cells, n);
            slots = std::max(slots, sl);
            if (far_context(cfg.flags)) { o.far_plan.push_back(pr.state_lo * g.G * g.G); o.far_plan.push_back(n); }
        }
        P.xfer2_cap = (single && cfg.world >= 4) ? 1024 : 0;       // (a ring of two or three has no rank beyond the neighbours)
        // A record for a rank further away: only a particle whose position stopped being a number travels that far (it is
        // filed under one fixed cell wherever it was), and only births make such particles (a child with the direction
        // (0, 0, 0)): with births on, a world of four or more all-gathers a small far outbox in the transfer phase.
        P.far_cap = (cfg.world >= 4 && (cfg.flags & PSAMD_FLAG_EXPLOSIONS)) ? 16 : 0;
        if (cfg.flags & PSAMD_FLAG_ALL_PAIRS) {
            P.allg_cells = cells;
            P.allg_cap = (int)((slots + 63) & ~(int64_t)63);
            P.allg_block = MSG_HEADER_WORDS + P.allg_cells + 4 * P.allg_cap;
        } else if (far_slab(cfg.flags)) {
            // 16 header | 4 or 10 planes (S, Sx, Sy, Sz; Sxx, Syy, Szz, Sxy, Sxz, Syz) of allg_cells doubles
            P.allg_cells = cells;
            P.allg_block = (int)(far_slab_block_bytes(far_planes(cfg.flags), cells) / sizeof(int));
        }
    }
    auto bits_for = [](int64_t n) { int b = 1; while (((int64_t)1 << b) < n) b++; return b; };
    P.key_chunk_shift = 2 + bits_for(g.container);
    P.key_rec_shift = P.key_chunk_shift + bits_for((int64_t)g.num_chunks + 1);
    P.key_bits = P.key_rec_shift + bits_for(g.queue_infos);
    {
        // (r.r + eps2)^3 over every pair of in-box positions, with slack for one wrap of drift
        const double lo = cfg.eps2 * cfg.eps2 * cfg.eps2, hi = std::pow(max_d2(g) + cfg.eps2, 3.0);
        // (scripts/field_bits.py's "probe-cutoff-8-generic" relies on eps2 = 1e-8 lying below this range: move the range, move the case)
        P.lean_math = (lo > std::ldexp(1.0, -60) && hi < std::ldexp(1.0, 60)) ? 1 : 0;
        // Collision flags before forces (lean modes): a collision needs two bodies within
        // COLLISION_RADIUS, so only bodies that close to a cell face concern the cell beyond it;
        // 2.5 % + 1e-3 of slack covers every rounding between here and the exact test.  Needs
        // the radius to be small against the cell (else the halo is the whole neighbour).
        P.halo_reach = (float)(cfg.collision_radius * 1.025 + 1e-3);
        {   // largest float t with (double)sqrtf(t) <= COLLISION_RADIUS (sqrtf: correctly rounded, monotone)
            auto collides = [&](float t) { return !((double)std::sqrt(t) > cfg.collision_radius); };
            uint32_t lo_b = 0u, hi_b = 0x7f7fffffu;                 // bit patterns of non-negative floats order like the floats
            auto as_f = [](uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; };
            if (!collides(0.0f)) P.coll_d2_max = -1.0f;
            else {
                while (lo_b < hi_b) { const uint32_t mid = lo_b + (hi_b - lo_b + 1) / 2; if (collides(as_f(mid))) lo_b = mid; else hi_b = mid - 1; }
                P.coll_d2_max = as_f(lo_b);
            }
        }
        P.two_pass = (P.lean_math && P.halo_reach < 0.25 * cfg.cell_size && !one_pass) ? 1 : 0;
    }
    if (P.key_bits > 63) return refuse(PSAMD_ERR_UNSUPPORTED, "queue-op key does not fit 64 bits for this configuration");
    if ((cfg.flags & PSAMD_FLAG_ALL_PAIRS) && !P.lean_math) return refuse(PSAMD_ERR_UNSUPPORTED, "all-pairs forces are built for the lean pair arithmetic only (EPS2 in its validated range)");
    if ((cfg.flags & PSAMD_FLAG_ALL_PAIRS) && !P.two_pass) return refuse(PSAMD_ERR_UNSUPPORTED, "all-pairs forces need the two-pass pair stage (collision radius small against the cell)");
    if ((cfg.flags & PSAMD_FLAG_FAR_QUADRUPOLE) && !(cfg.flags & PSAMD_FLAG_FAR_PYRAMID))
        return refuse(PSAMD_ERR_INVALID_ARG, "quadrupoles (PSAMD_FLAG_FAR_QUADRUPOLE) belong to the pyramid of monopoles: set PSAMD_FLAG_FAR_PYRAMID too");
    if (far_context(cfg.flags)) {
        // (both flags: what the flat method refuses comes first, then the choice between the two)
        const bool mono = (cfg.flags & PSAMD_FLAG_FAR_MONOPOLE) != 0, pyr = (cfg.flags & PSAMD_FLAG_FAR_PYRAMID) != 0;
        const std::string who = mono ? "far monopoles" : "the pyramid of monopoles", is = mono ? " are " : " is ";
        const char *two = "far monopoles and all-pairs forces are two force models: choose one";
        const char *three = "the pyramid of monopoles, far monopoles and all-pairs forces are three force models: choose one";
        if (cfg.flags & PSAMD_FLAG_ALL_PAIRS) return refuse(PSAMD_ERR_INVALID_ARG, mono ? two : three);
        if (cfg.world > 1 && !(cfg.flags & PSAMD_FLAG_FAR_SLAB))
            return refuse(PSAMD_ERR_UNSUPPORTED, who + is + "served on one context only (world == 1)");
        if (!P.lean_math) return refuse(PSAMD_ERR_UNSUPPORTED, who + is + "built for the lean pair arithmetic only (EPS2 in its validated range)");
        if (!P.two_pass) return refuse(PSAMD_ERR_UNSUPPORTED, who + (mono ? " need" : " needs") + " the two-pass pair stage (collision radius small against the cell)");
        if (mono && pyr) return refuse(PSAMD_ERR_INVALID_ARG, three);
        o.lev = pyr ? far_levels_of(g.G) : far_one_level(g.G);
    }
    for (int k = 0; k < 5; k++) { o.S.seg_base[k] = g.seg_base[k]; o.S.info_base[k] = g.info_base[k]; }
    for (int k = 0; k < 4; k++) o.S.seg_size_t[k] = g.seg_size_t[k];
    P.eps2f = (float)cfg.eps2;
    P.eps_f32_from = INFINITY;   // always add EPS2 in double, unless probe_eps_f32 finds a threshold
    split_interior(g, o);
    size_arrays_and_msgs(g, o);
    return PSAMD_OK;
}

}  // namespace psamd
