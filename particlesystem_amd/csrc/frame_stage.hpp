// frame_stage.hpp -- where the host stands inside a frame: one stage, the calls that read or move it, one table.
// Host only and free of HIP: any C++17 compiler takes it (tests/test_frame_stage_cpu.py walks the whole table).
//
// A frame is PLAIN (init_iframe, build_grid, calc_forces' two halves; psamd_step is a whole one) or SLAB (slab_build
// ... slab_finish) from its build to its end.  A context of a world of one may be stepped by either family, frame by
// frame; a context that is one slab of several takes the slab calls only (step.hip refuses the others before it asks here).
#pragma once

namespace psamd {

enum Stage : unsigned {
    ST_IDLE = 0,        // between frames
    ST_RESET,           // init_iframe has run
    ST_BUILT,           // build_grid
    ST_PAIRS,           // calc_forces_pairs
    ST_SLAB_BUILT,      // slab_build
    ST_SLAB_INTERIOR,   // ... and slab_pairs_interior has run its pass
    ST_SLAB_PAIRS,      // slab_pairs
    ST_SLAB_APPLIED,    // slab_apply
    ST_COUNT
};

enum Call : unsigned {
    CALL_INIT_IFRAME = 0, CALL_BUILD_GRID, CALL_PAIRS, CALL_APPLY, CALL_STEP,
    CALL_SLAB_BUILD, CALL_SLAB_INTERIOR, CALL_SLAB_PAIRS, CALL_SLAB_APPLY, CALL_SLAB_FINISH,
    CALL_CHANGED,       // the slots or the queues changed under the frame: fill, upload, inject, remove
    CALL_RESTORE,       // snapshot_restore
    CALL_COUNT
};

constexpr unsigned bit(Stage s) { return 1u << s; }
constexpr unsigned ST_PLAIN = bit(ST_BUILT) | bit(ST_PAIRS);
constexpr unsigned ST_SLAB = bit(ST_SLAB_BUILT) | bit(ST_SLAB_INTERIOR) | bit(ST_SLAB_PAIRS) | bit(ST_SLAB_APPLIED);
constexpr unsigned ST_OPEN = bit(ST_IDLE) | bit(ST_RESET);     // no frame built: either family may build one
constexpr unsigned ST_ANY = ST_OPEN | ST_PLAIN | ST_SLAB;

struct StageRow {
    unsigned from;      // the stages the call is accepted from
    unsigned other;     // stages of the other family's frame the order test alone would let it through: refused as mixed
    unsigned keeps;     // accepted from these, the call leaves the stage as it is
    Stage to;           // ... from the others, the stage it leaves
    Stage failed;       // the stage after a failed enqueue (ST_COUNT: as it was)
    const char *refusal;
};

constexpr const char *MIXED_REFUSAL =
    "a frame is stepped by one family of calls from its build to its end: init_iframe / build_grid / calc_forces / step, "
    "or slab_build / _pairs / _apply / _finish";

constexpr StageRow STAGE_TABLE[CALL_COUNT] = {
    /* init_iframe   */ {ST_OPEN | ST_PLAIN, ST_SLAB, 0, ST_RESET, ST_COUNT, ""},
    /* build_grid    */ {bit(ST_RESET), 0, 0, ST_BUILT, ST_COUNT, "build_grid needs init_iframe first"},
    /* pairs         */ {ST_PLAIN, ST_SLAB, 0, ST_PAIRS, ST_COUNT, "calc_forces needs build_grid first"},
    /* apply         */ {bit(ST_PAIRS), bit(ST_SLAB_PAIRS) | bit(ST_SLAB_APPLIED), 0, ST_IDLE, ST_COUNT, "apply needs build_grid and the pair pass first"},
    /* step          */ {ST_OPEN | ST_PLAIN, ST_SLAB, 0, ST_IDLE, ST_COUNT, ""},
    /* slab_build    */ {ST_OPEN | ST_SLAB, ST_PLAIN, 0, ST_SLAB_BUILT, ST_COUNT, ""},
    /* slab_interior */ {bit(ST_SLAB_BUILT) | bit(ST_SLAB_INTERIOR), 0, 0, ST_SLAB_INTERIOR, ST_COUNT, "slab_pairs_interior belongs between slab_build and slab_pairs"},
    /* slab_pairs    */ {bit(ST_SLAB_BUILT) | bit(ST_SLAB_INTERIOR), 0, 0, ST_SLAB_PAIRS, ST_SLAB_BUILT, "slab_pairs needs slab_build (and the halo exchange) first"},
    /* slab_apply    */ {bit(ST_SLAB_PAIRS), 0, 0, ST_SLAB_APPLIED, ST_COUNT, "slab_apply needs slab_pairs (and the force exchange) first"},
    /* slab_finish   */ {bit(ST_SLAB_APPLIED), 0, 0, ST_IDLE, ST_COUNT, "slab_finish needs slab_apply (and the transfer exchange) first"},
    /* changed       */ {ST_ANY, 0, bit(ST_RESET), ST_IDLE, ST_COUNT, ""},
    /* restore       */ {ST_ANY, 0, 0, ST_IDLE, ST_COUNT, ""},
};

// the order test: nullptr if the call is accepted from this stage, else why not
constexpr const char *enter(Stage s, Call k)
{
    const StageRow &r = STAGE_TABLE[k];
    return (r.from & bit(s)) ? nullptr : (r.other & bit(s)) ? MIXED_REFUSAL : r.refusal;
}

// an accepted call is over: the stage it leaves behind
constexpr void leave(Stage &s, Call k, bool ok = true)
{
    const StageRow &r = STAGE_TABLE[k];
    if (!ok) { if (r.failed != ST_COUNT) s = r.failed; }
    else if (!(r.keeps & bit(s))) s = r.to;
}

// ---- what the other calls ask of the stage ----
constexpr bool built(Stage s) { return ((ST_PLAIN | ST_SLAB) & bit(s)) != 0; }                                     // the grid lists are the frame's
constexpr bool pairs_done(Stage s) { return ((bit(ST_PAIRS) | bit(ST_SLAB_PAIRS) | bit(ST_SLAB_APPLIED)) & bit(s)) != 0; }
constexpr bool interior_passed(Stage s) { return s == ST_SLAB_INTERIOR; }
// potential and probe: a frame is built, its particles have not moved, and -- a slab of several -- the halos are in
constexpr bool field_window(Stage s, int world) { return world > 1 ? s == ST_SLAB_PAIRS : built(s) && s != ST_SLAB_APPLIED; }
// update: a slot still holds the particle that the caller means -- between slab_apply and slab_finish the departing ones are staged
constexpr bool update_window(Stage s) { return s != ST_SLAB_APPLIED; }

}  // namespace psamd
