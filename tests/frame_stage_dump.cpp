// Prints the whole of csrc/frame_stage.hpp for tests/test_frame_stage_cpu.py: per (stage, call) what the table
// answers, per stage the predicates.  Host only; the test builds it with the address and undefined-behaviour sanitizers.
#include <cstdio>

#include "frame_stage.hpp"

using namespace psamd;

static const char *const STAGES[ST_COUNT] = {"IDLE", "RESET", "BUILT", "PAIRS", "SLAB_BUILT", "SLAB_INTERIOR", "SLAB_PAIRS", "SLAB_APPLIED"};
static const char *const CALLS[CALL_COUNT] = {"init_iframe", "build_grid", "calc_forces_pairs", "calc_forces_apply", "step", "slab_build",
                                              "slab_pairs_interior", "slab_pairs", "slab_apply", "slab_finish", "changed", "snapshot_restore"};

int main()
{
    for (unsigned s = 0; s < ST_COUNT; s++)
        for (unsigned k = 0; k < CALL_COUNT; k++) {
            const char *why = enter((Stage)s, (Call)k);
            if (why) { std::printf("T %s %s refuse %s\n", STAGES[s], CALLS[k], why == MIXED_REFUSAL ? "mixed" : "order"); continue; }
            Stage ok = (Stage)s, failed = (Stage)s;
            leave(ok, (Call)k);
            leave(failed, (Call)k, false);
            std::printf("T %s %s %s %s\n", STAGES[s], CALLS[k], STAGES[ok], STAGES[failed]);
        }
    for (unsigned s = 0; s < ST_COUNT; s++)
        std::printf("P %s %d %d %d %d %d\n", STAGES[s], (int)built((Stage)s), (int)pairs_done((Stage)s), (int)interior_passed((Stage)s),
                    (int)field_window((Stage)s, 1), (int)field_window((Stage)s, 2));
    for (unsigned k = 0; k < CALL_COUNT; k++) std::printf("R %s %s\n", CALLS[k], STAGE_TABLE[k].refusal);
    std::printf("M %s\n", MIXED_REFUSAL);
    return 0;
}
