// frame_scalars.h -- the per-frame scalar record, the step's own state on the device and the sticky error bits: what the
// kernels publish and the host's ledger of steps (step_ledger.hpp) reads.  Plain integers, free of HIP.
#pragma once
#include <cstdint>

namespace psamd {
// Per-frame scalars living in device memory (zeroed by init_iframe).
struct FrameScalars {
    int32_t gridmax[2];     // hostGridMax: biggest chunk, biggest cell (ps.cpp:76)
    int32_t live;           // particles with a valid cell at build_grid
    int32_t error;          // sticky bit mask, see ERR_* below
    int32_t n_ops;          // queue operations emitted by apply   \ allocated together as one
    int32_t n_moves;        // relocation / birth records emitted  / 64-bit word (ops low)
    int32_t max_bucket;     // most queue operations any one segment received this step
    int32_t n_tasks;        // non-empty (cell, slice) tasks of the pair kernel this frame
    int32_t n_tasks2;       // two-pass mode: (cell, 64-slice) tasks over the particles that need a force
    int32_t n_merged;       // ... and merged tasks (up to four cells' partly filled last slices in one wave)
    int32_t n_out[5];       // slab mode: relocation / birth records leaving for the rank below [0] / above [1], two ranks below [2] / above [3], any other rank [4] (the all-gathered far outbox)
    int32_t n_lent;         // slab mode: bodies in the lent-in region this frame
    int32_t chunk_over;     // a chunk's count passed MAX_PARTICLES_PER_CHUNK this frame: the tail of its list is skipped (k_chunk_cap)
    int32_t status_error;   // slab mode: OR of the error bits in this step's all-gathered status records (every rank sees the same word)
    int32_t seq;            // host copy only: the number of the step whose scalars these are, written last (the host polls it)
    int32_t max_cell_raw;   // most ids any own cell received this frame, uncapped (gridmax[1] is capped at the list capacity)
    int32_t xfer_cap_next;  // slab mode: the transfer messages' capacity every rank adopts two steps on (k_status_merge: the same number on every rank)
    int32_t pad_fs;
    long long cost_total;   // two-pass mode: sum over the force pass's tasks of the bodies each walks (its stencil's population)
};
static_assert(sizeof(FrameScalars) == 96 && __builtin_offsetof(FrameScalars, seq) == 72 && __builtin_offsetof(FrameScalars, cost_total) == 88, "one layout");

// What a step needs to know about its own number, kept on the device so that no kernel argument changes from
// one step to the next (a captured hipGraph replays the arguments it was captured with): `step` keys the
// explosion RNG (k_apply, k_replay_commit's commit_move), `seq` counts the scalar records handed to the host.  The workgroup
// that publishes a step's scalars raises `pending`; the next frame's first kernel (k_hist_lds) -- nothing reads `step`
// while it runs -- turns that into step + 1.  snapshot_restore rewinds `step` (k_restore).
struct StepState {
    int32_t step, pending, seq;
    int32_t last_departures;   // slab mode: most records this rank sent in one direction in the step before (goes out with the next status record)
    int32_t peak_prev, pad_st; // slab mode: the busiest rank's count in the status records of the step before (the same number on every rank)
    // The balanced force pass paces its waves against the clock (balanced.hpp, WavePace): per pass of a frame (0 / 1), when
    // the pass's planning ended (100 MHz real-time counter), when its last wave ended, and how long the last such pass
    // took -- what this one expects to take.
    unsigned long long pairs_t0[2], pairs_end[2];
    int32_t pairs_ticks[2];
};

enum : int32_t {
    ERR_CELL_TOO_BIG = 1,   // (not raised since round 5: k_sort_cells ranks a cell of any size, through global memory beyond its LDS room; the bit and its message stay for ABI stability)
    ERR_BAD_ID = 2,         // uploaded P_DATA_TYPE with id != slot
    ERR_OPS_OVERFLOW = 4,   // lifecycle op buffer too small
    ERR_BAD_POS = 16,       // uploaded live particle outside the box (or cell out of range)
    ERR_FOREIGN_CELL = 32,  // slab mode: a particle stored here sits in a layer this rank holds no state for
    ERR_HALO_OVERFLOW = 64, // slab mode: a halo / force / relocation message had no room for what it must carry
    ERR_SLAB_MISMATCH = 128,// slab mode: a message disagrees with the receiver's own counts
    ERR_REMOTE_RECORD0 = 256,// slab mode: a cell-overflow kill on a rank that does not own queue record 0
    ERR_CHUNK_CAP = 512,    // a chunk list passed MAX_PARTICLES_PER_CHUNK (the reference would skip its tail)
    ERR_HANDOFF_TIMEOUT = 1024, // force pass: a wave never saw the partial sums of the task it continues (should be impossible)
};

}  // namespace psamd
