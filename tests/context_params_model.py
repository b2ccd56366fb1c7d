"""What context creation derives before it touches the device, restated from the rules (include/psamd.h, the
comments of csrc/device_types.h) in Python and numpy: the model tests/test_context_params_cpu.py holds
csrc/context_params.hpp against, and tests/test_gpu_context_params.py a real context.

derive(cfg, sizes, plans, one_pass) takes the configuration, the geometry's numbers as psamd_describe gives them (Sizes) and
every rank's plan as psamd_slab_plan_describe gives it (None: that rank has none).  It returns a status (a refusal) or a
dict: field name -> list of integers, floats and doubles as their bits."""
import math

import numpy as np

OK, INVALID_ARG, UNSUPPORTED = 0, 1, 9
EXPLOSIONS, ALL_PAIRS, FAR_MONOPOLE, FAR_PYRAMID, FAR_QUADRUPOLE, FAR_SLAB = 0x1, 0x4, 0x10, 0x20, 0x40, 0x80
MAX_RANKS = 64
HEADER_WORDS, XFER_REC_WORDS, KILL_CAP = 16, 16, 4080     # a message's header; a transfer record is 64 bytes; kills a status record lists
INT32_MAX = 2 ** 31 - 1
(HALO_OUT, HALO_IN, FORCE_OUT, FORCE_IN, XFER_OUT, XFER_IN, STATUS_OUT, STATUS_IN, ALLG_OUT, ALLG_IN, XFER2_OUT, XFER2_IN,
 FAR_OUT, FAR_IN, MSG_COUNT) = 0, 2, 4, 5, 6, 8, 10, 11, 12, 13, 14, 16, 18, 19, 20
F32_INF = np.float32(np.inf)


def bits32(x):
    return int(np.float32(x).view(np.uint32))


def bits64(x):
    return int(np.float64(x).view(np.uint64))


def up(f):
    return np.nextafter(np.float32(f), F32_INF)


def down(f):
    return np.nextafter(np.float32(f), -F32_INF)


def at_least(v):
    """the smallest float that is >= the double v"""
    f = np.float32(v)
    return up(f) if float(f) < v else f


def at_most(v):
    """the largest float that is <= the double v"""
    f = np.float32(v)
    return down(f) if float(f) > v else f


def largest_colliding_d2(radius):
    """The largest float whose square root (fp32, correctly rounded), taken as a double, does not exceed the radius -- the
    float above it does; -1 where not even 0 qualifies."""
    def within(t):
        return not float(np.sqrt(np.float32(t))) > radius
    if not within(0.0):
        return np.float32(-1.0)
    t = np.float32(radius) * np.float32(radius)     # a float nearby, then walked to the edge
    while not within(t):
        t = down(t)
    while within(up(t)):
        t = up(t)
    assert within(t) and not within(up(t))
    return t


def bits_for(n):
    b = 1
    while (1 << b) < n:
        b += 1
    return b


def group_of_layer(i3, D):
    k, r = divmod(i3, D)
    return 2 * k if r == 0 else 2 * (k + 1) if r == D - 1 else 2 * k + 1


def far_levels(G, pyramid):
    dims, off = [], [0]
    g = G
    while True:
        dims.append(g)
        off.append(off[-1] + (g ** 3 + 63) // 64 * 64)
        if not pyramid or g <= 4 or len(dims) == 10:
            break
        g = (g + 1) // 2
    return dims, off


def xfer_bytes(recs):
    return 4 * (HEADER_WORDS + recs * XFER_REC_WORDS)


def model_of(cfg, one_pass=False):
    """derive() on what the library's two host-only descriptions say of cfg (neither needs a GPU)"""
    import ctypes as C

    import particlesystem_amd as ps
    sizes = ps.Sizes()
    assert ps.load().psamd_describe(C.byref(cfg), C.byref(sizes), None, None, None, None) == 0
    plans = []
    for r in range(cfg.world if 1 <= cfg.world <= MAX_RANKS else 0):
        other = type(cfg).from_buffer_copy(cfg)
        other.rank = r
        try:
            plans.append(ps.slab_plan(other))
        except ps.PsamdError:
            plans.append(None)
    return derive(cfg, sizes, plans, one_pass)


def derive(cfg, sizes, plans, one_pass=False):
    world, rank, flags = cfg.world, cfg.rank, cfg.flags
    far = bool(flags & (FAR_MONOPOLE | FAR_PYRAMID))
    far_slab = far and bool(flags & FAR_SLAB)
    allp = bool(flags & ALL_PAIRS)
    # ---- the refusals that need no arithmetic, in the order the library makes them
    if not (1 <= world <= MAX_RANKS and 0 <= rank < world):
        return INVALID_ARG
    if plans[rank] is None:
        return UNSUPPORTED
    if cfg.drag < 0:
        return INVALID_ARG
    if (flags & FAR_SLAB) and not far:
        return INVALID_ARG
    if world > 1 and any(p is None for p in plans):
        return UNSUPPORTED
    pl = plans[rank]
    G, D, F = sizes.grid_dim, cfg.chunk_dim, cfg.chunk_factor
    GG, mpc = G * G, sizes.max_per_cell
    seg_count, seg_size_t, seg_size = list(sizes.seg_count), list(sizes.seg_size_t), list(sizes.seg_size)
    nrec, nchunks = sizes.queue_info_size, sizes.num_chunks
    out = {}
    out["plan"] = [world, rank, G, D, F, pl.cut_lo, pl.cut_hi, pl.state_lo, pl.state_hi, group_of_layer(pl.state_lo, D),
                   group_of_layer(pl.state_hi - 1, D) + 1, pl.below_lo, pl.below_hi, pl.above_lo, pl.above_hi, pl.lentin_lo, pl.lentin_hi,
                   pl.lentout_lo, pl.lentout_hi, pl.send_up_lo, pl.send_up_hi, pl.send_down_lo, pl.send_down_hi,
                   (rank + 1) % world if world > 1 else -1, (rank - 1) % world if world > 1 else -1, 1]
    for f in ("slot_lo", "slot_hi", "rec_lo", "rec_hi"):
        out["plan." + f] = list(getattr(pl, f))
    # ---- the physics' constants
    life = cfg.life_steps * cfg.dt
    kid_age = life / 10.0
    radius = cfg.collision_radius
    L = float(G) * cfg.cell_size
    d2_most = 3.0 * (2.0 * L) * (2.0 * L)
    lean = cfg.eps2 * cfg.eps2 * cfg.eps2 > 2.0 ** -60 and math.pow(d2_most + cfg.eps2, 3.0) < 2.0 ** 60
    reach = np.float32(radius * 1.025 + 1e-3)
    two_pass = lean and float(reach) < 0.25 * cfg.cell_size and not one_pass
    out.update({
        "P.G": [G], "P.num_cells": [sizes.num_cells], "P.num_chunks": [nchunks], "P.container": [sizes.container_size],
        "P.max_per_cell": [mpc], "P.max_per_chunk": [sizes.max_per_chunk], "P.slices": [-(-mpc // 64)], "P.flags": [flags],
        "P.t": [bits32(cfg.dt)], "P.kid_thr": [bits32(at_least(kid_age))], "P.life_thr": [bits32(at_most(life))],
        "P.coll_d2_gate": [bits32(radius * radius * 1.001 + 1e-30)],
        "P.dmax": [bits32(cfg.cell_size)], "P.vmax": [bits32(cfg.max_v)], "P.w_default": [bits32(cfg.particle_weight)],
        "P.fert_lo": [bits32(life / 6.0)], "P.fert_hi": [bits32(life * 2.0)],
        "P.cell_size": [bits64(cfg.cell_size)], "P.eps2": [bits64(cfg.eps2)], "P.coll_radius": [bits64(radius)],
        "P.kid_age": [bits64(kid_age)], "P.life": [bits64(life)], "P.expl_speed": [bits64(cfg.explosion_speed)],
        "P.seed": [cfg.seed],
        "P.lean_math": [int(lean)], "P.eps2f": [bits32(cfg.eps2)], "P.eps_f32_from": [bits32(np.inf)], "P.slow_below": [0],
        "P.halo_reach": [bits32(reach)], "P.coll_d2_max": [bits32(largest_colliding_d2(radius))], "P.two_pass": [int(two_pass)], "P.pad_f": [0],
        "P.drag": [bits32(cfg.drag)], "P.force_sign": [bits32(-1.0 if cfg.force_sign < 0 else 1.0)],
    })
    shift_chunk = 2 + bits_for(sizes.container_size)
    shift_rec = shift_chunk + bits_for(nchunks + 1)
    out["P.key_chunk_shift"], out["P.key_rec_shift"], out["P.key_bits"] = [shift_chunk], [shift_rec], [shift_rec + bits_for(nrec)]
    # ---- what the rank holds: four regions of whole layers (own, halo below, lent in, halo above), a gap cell behind each
    first = [pl.state_lo, pl.below_lo, pl.lentin_lo, pl.above_lo]
    layers = [pl.state_hi - pl.state_lo, pl.lentin_lo - pl.below_lo, pl.lentin_hi - pl.lentin_lo, pl.above_hi - pl.above_lo]
    halo_cap = cfg.halo_cap_cell if 0 < cfg.halo_cap_cell < mpc else mpc
    slot_n = [pl.slot_hi[t] - pl.slot_lo[t] for t in range(4)]
    slots = sum(slot_n)
    cells_of = np.array(layers) * GG
    base = np.concatenate([[0], np.cumsum(cells_of + 1)])
    room = [slots] + [int(c) * halo_cap for c in cells_of[1:]]
    sorted_at = np.concatenate([[0], np.cumsum(room)])
    comp0 = (max(pl.cut_lo, pl.state_lo) - pl.state_lo) * GG
    comp1 = max(comp0, (min(pl.cut_hi, pl.state_hi) - pl.state_lo) * GG)
    if world > 1:
        xfer_cap = cfg.xfer_cap if cfg.xfer_cap > 0 else max(4096, GG * mpc // 4)
        xfer_max = max(xfer_cap, cfg.xfer_cap_max if cfg.xfer_cap_max > 0 else min(4 * GG * mpc, INT32_MAX // 256))
    else:
        xfer_cap = xfer_max = 0
    comp_lo, comp_hi = [int(base[2]), comp0, 0], [int(base[2]) + int(cells_of[2]), comp1, 0]
    lentout = [(pl.lentout_lo - pl.state_lo) * GG, (pl.lentout_hi - pl.state_lo) * GG]
    out.update({
        "P.reg_first": first, "P.reg_layers": layers, "P.reg_base": [int(b) for b in base[:4]], "P.reg_sorted": [int(s) for s in sorted_at[:4]],
        "P.n_local_cells": [int(base[4])], "P.n_own_cells": [int(cells_of[0])], "P.sorted_cap": [int(sorted_at[4])],
        "P.own_comp0": [comp0], "P.own_comp1": [comp1], "P.comp_lo": comp_lo, "P.comp_hi": comp_hi,
        "P.slot_lo": list(pl.slot_lo), "P.slot_n": slot_n, "P.slots_total": [slots], "P.rec_lo": list(pl.rec_lo), "P.rec_hi": list(pl.rec_hi),
        "P.rank": [rank], "P.world": [world], "P.halo_cap_cell": [halo_cap],
        "P.xfer_cap": [xfer_cap], "P.xfer_cap_max": [xfer_max], "P.xfer_cap0": [xfer_cap],
        "P.lentout_c0": [lentout[0]], "P.lentout_c1": [lentout[1]], "P.num_cells_global": [sizes.num_cells],
        "P.status_words": [16 + KILL_CAP + 4 * nchunks],
    })
    # ---- what the other ranks are to this one
    nbr_lo, nbr_hi = [0] * 8, [0] * 8
    xfer2 = far_cap = allg_cells = allg_cap = allg_block = 0
    far_plan = []
    if world > 1:
        for side, r in enumerate(((rank - 1) % world, (rank + 1) % world)):
            nbr_lo[4 * side:4 * side + 4] = list(plans[r].rec_lo)
            nbr_hi[4 * side:4 * side + 4] = list(plans[r].rec_hi)
        state_cells = [(p.state_hi - p.state_lo) * GG for p in plans]
        most_slots = max(sum(p.slot_hi[t] - p.slot_lo[t] for t in range(4)) for p in plans)
        if world >= 4 and min(p.state_hi - p.state_lo for p in plans) < 2:
            xfer2 = 1024
        if world >= 4 and flags & EXPLOSIONS:
            far_cap = 16
        if allp:
            allg_cells, allg_cap = max(state_cells), (most_slots + 63) // 64 * 64
            allg_block = HEADER_WORDS + allg_cells + 4 * allg_cap
        elif far_slab:
            allg_cells = max(state_cells)
            allg_block = (64 + (10 if flags & FAR_QUADRUPOLE else 4) * allg_cells * 8) // 4
        if far:
            far_plan = [v for p, n in zip(plans, state_cells) for v in (p.state_lo * GG, n)]
    out.update({"P.nbr_rec_lo": nbr_lo, "P.nbr_rec_hi": nbr_hi, "P.xfer2_cap": [xfer2], "P.far_cap": [far_cap],
                "P.allg_cells": [allg_cells], "P.allg_cap": [allg_cap], "P.allg_block": [allg_block], "far_plan": far_plan})
    # ---- the refusals that follow from the arithmetic
    if shift_rec + bits_for(nrec) > 63:
        return UNSUPPORTED
    if allp and not (lean and two_pass):
        return UNSUPPORTED
    if (flags & FAR_QUADRUPOLE) and not (flags & FAR_PYRAMID):
        return INVALID_ARG
    if far:
        if allp:
            return INVALID_ARG
        if world > 1 and not (flags & FAR_SLAB):
            return UNSUPPORTED
        if not (lean and two_pass):
            return UNSUPPORTED
        if (flags & FAR_MONOPOLE) and (flags & FAR_PYRAMID):
            return INVALID_ARG
    dims, off = far_levels(G, bool(flags & FAR_PYRAMID)) if far else ([], [0])
    out["lev.n"] = [len(dims)]
    out["lev.G"] = dims + [0] * (10 - len(dims))
    out["lev.off"] = off + [0] * (11 - len(off))
    seg_base = [0] + [int(v) for v in np.cumsum(seg_size)]
    out["S.seg_base"], out["S.info_base"], out["S.seg_size_t"] = seg_base, [0] + [int(v) for v in np.cumsum(seg_count)], seg_size_t
    # ---- the interior: the first run of computed own layers whose two neighbour layers are own state or outside the grid
    lo, hi = max(pl.cut_lo, pl.state_lo), min(pl.cut_hi, pl.state_hi)
    def mine(l):
        return l < 0 or l >= G or pl.state_lo <= l < pl.state_hi
    inner = [l for l in range(lo, hi) if mine(l - 1) and mine(l + 1)]
    run = [l for k, l in enumerate(inner) if l == inner[0] + k]
    have = (world > 1 and two_pass and lean and len(run) > 0 and len(run) < (hi - lo) + (pl.lentin_hi - pl.lentin_lo)
            and not (allp or far))
    out["have_interior"] = [int(have)]
    if have:
        a, b = (run[0] - pl.state_lo) * GG, (run[-1] + 1 - pl.state_lo) * GG
        out["int_lo"], out["int_hi"] = [a, 0, 0], [b, 0, 0]
        out["rest_lo"], out["rest_hi"] = [comp_lo[0], comp0, b], [comp_hi[0], a, comp1]
    else:
        out["int_lo"] = out["rest_lo"] = comp_lo
        out["int_hi"] = out["rest_hi"] = comp_hi
    # ---- the sizes of the step's lists and of the messages
    LC = int(base[4])
    room_recs = xfer_max + xfer2 + far_cap * max(1, world) // 2 + 1
    out["xfer_room"] = [room_recs]
    out["ops_cap"] = [min(3 * slots + 2 * room_recs + 64 + (world * KILL_CAP if world > 1 else 0), INT32_MAX // 2)]
    out["moves_cap"] = [min(2 * slots + 2 * room_recs + 64, INT32_MAX // 2)]
    out["frame_ints"] = [3 * LC + nchunks + 2 * nrec + 2 * LC * -(-mpc // 64)]
    msg = [(0, 0)] * MSG_COUNT
    halo_out_cells = halo_out_c0 = halo_in_cells = [0, 0]
    if world > 1:
        halo_out_cells = [(pl.send_down_hi - pl.send_down_lo) * GG, (pl.send_up_hi - pl.send_up_lo) * GG]
        halo_out_c0 = [(pl.send_down_lo - pl.state_lo) * GG, (pl.send_up_lo - pl.state_lo) * GG]
        halo_in_cells = [(pl.below_hi - pl.below_lo) * GG, (pl.above_hi - pl.above_lo) * GG]

        def put(which, nbytes, alloc=None):
            msg[which] = (nbytes, nbytes if alloc is None else alloc)

        def halo(cells):       # the header, a count per cell, six words a body
            return 4 * (HEADER_WORDS + cells + 6 * cells * halo_cap)

        def force(cells):      # the header, four words a body
            return 4 * (HEADER_WORDS + 4 * cells * halo_cap)
        for k in (0, 1):
            if halo_out_cells[k] > 0:
                put(HALO_OUT + k, halo(halo_out_cells[k]))
            if halo_in_cells[k] > 0:
                put(HALO_IN + k, halo(halo_in_cells[k]))
            put(XFER_OUT + k, xfer_bytes(xfer_cap + 1), xfer_bytes(room_recs))
            put(XFER_IN + k, xfer_bytes(xfer_cap + 1), xfer_bytes(room_recs))
            if xfer2:
                put(XFER2_OUT + k, xfer_bytes(xfer2))
                put(XFER2_IN + k, xfer_bytes(xfer2))
        if layers[2] > 0:
            put(FORCE_OUT, force(layers[2] * GG))
        if lentout[1] > lentout[0]:
            put(FORCE_IN, force(lentout[1] - lentout[0]))
        if far_cap:
            put(FAR_OUT, xfer_bytes(far_cap))
            put(FAR_IN, xfer_bytes(far_cap) * world)
        if allp or far_slab:
            put(ALLG_OUT, 4 * allg_block)
            put(ALLG_IN, 4 * allg_block * world, 4 * allg_block * world + (256 if allp else 0))    # all-pairs: 64 words of slack
        put(STATUS_OUT, 4 * out["P.status_words"][0])
        put(STATUS_IN, 4 * out["P.status_words"][0] * world)
    out["halo_out_c0"], out["halo_out_cells"], out["halo_in_cells"] = halo_out_c0, halo_out_cells, halo_in_cells
    for w in range(MSG_COUNT):
        out["msg.%d" % w] = list(msg[w])
    return out
