// step_ledger.hpp -- the host's ledger of steps: which steps it has enqueued, which of their scalar records it has read,
// and everything it derives from the records -- the hints that size the launches to come, the counters, the verdicts.
// Host only and free of HIP: any C++17 compiler takes it (tests/test_step_ledger_cpu.py walks it beside a restatement
// of the statements it replaced).  Waiting for a record, fetching an error's text and the launches stay in step.hip.
//
// THE PIPELINE.  Nothing in a step waits for the host: the step's tail decides everything on the device, and the one
// read-back of a step -- live count, sticky errors, list sizes: what the reference's driver fetches as hostGridMax,
// ps.cpp:1878-1900 -- is a FrameScalars record the last bucketing workgroup stores into pinned host memory, its number
// (`seq`) last.  The device numbers the records it hands out (StepState.seq); the ledger counts the steps enqueued
// (seq()) and the records read (seen()).  There are TWO pinned records and a step's number picks one (s & 1), so the
// record of step s - 2 must have been read when step s can publish.  run_ahead = 1: the call that enqueues step s
// reads the record of step s - 1, waiting for it, and that of step s too if it has arrived already -- the host is
// never on a step's critical path; run_ahead = 0: every step's own record is waited for before the call returns.
// Either way a step is enqueued with at most one record unread and never more than two are outstanding (run-ahead is
// at most 1: the two pinned records would not carry more).
//
// HINTS come from the last record READ, which with run-ahead is not the last step's: every unread step may have added a
// child per particle (explosions on) and a slab its arrivals, so alive_at_most() doubles per unread step and adds the
// messages' room.  It is an upper bound of the particles alive at the next build_grid WHATEVER is in flight
// (tests/test_step_ledger_cpu.py holds it to a simulated population): a call that changes the particles between two
// steps -- fill, inject, upload, snapshot_restore -- is booked under the last step enqueued, and the record of that step
// or of an earlier one, read afterwards, speaks of the particles before the call: a fill or an inject is added to what
// such a record says (tally_), after an upload or a restore such a record leaves the bound alone and only a later step's
// sets it again (reset_step_).  The far walks and their combine size a launch from the bound that should cover every
// particle (far_dense_bound; they go by the device's own count in rounds, so a launch that is too small would cost
// time, not particles); every other figure is a hint whose miss only costs time.  The other hints (tasks, packs, the
// longest list, last_live()) follow the last record read as they are: stale by a call for a step or two, then right.
//
// VERDICTS.  A record that carries error bits asks for a verdict (absorb() says so; step.hip fetches the status and
// its text).  The first verdict of a reading call is held (hold_verdict) and released by the next call that reports
// verdicts (take_verdict): the stage call that read it, or psamd_synchronize after a call that reads quietly
// (psamd_get_counters).  A slab fails COLLECTIVELY: only on error bits that were in a step's all-gathered status
// records, which every rank sees alike (status_error).  An error this rank raised after its status record was closed
// (a message that did not fit, an arrival for a queue it does not hold) stays sticky on the device, goes out with the
// next step's record and stops every rank there; returning it at once would leave the ranks that have not heard of
// it waiting in the next exchange.
//
// CAPACITY.  The transfer messages' capacity all ranks agreed on in step s (xfer_cap_next: an absolute number, the same
// on every rank) takes effect in step s + 2 on every rank: the record of step s - 2 has been read by every host that
// starts step s, whatever its run-ahead (adopt_cap).
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <set>
#include <string>

#include "frame_scalars.h"

namespace psamd {

// the integers of the context the ledger's rules read (context.hpp: ledger_params)
struct LedgerParams {
    int64_t slots_total;
    bool explosions;
    int world, xfer_cap, xfer2_cap, far_cap;     // records a transfer / two-rank / far message carries now
    int xfer_cap0, xfer_cap_max;                 // the bounds of xfer_cap
    int comp, comp_int, comp_rest;               // cells the whole pair stage computes; its interior pass; the pass after it
    int64_t kill_room;                           // cell-overflow kills a step's status records can bring in (0: one rank)
    int bucket_max;                              // the longest operation list the largest replay instance sorts in LDS
};

class StepLedger {
public:
    // ---- the step engine ----
    void set_run_ahead(int steps) { run_ahead_ = steps; }
    void interior_pass_ran() { interior_ran_ = true; }      // the frame in progress runs its pair stage in two passes
    int enqueued()                                          // a step was enqueued: its number
    {
        if (interior_ran_) interior_steps_.insert(seq_ + 1);
        interior_ran_ = false;
        return ++seq_;
    }
    int seq() const { return seq_; }
    int seen() const { return seen_; }
    int due() const { return run_ahead_ ? seq_ - 1 : seq_; }    // the record the call that enqueued step seq() waits for
    // a launch failed between a record's publishing and enqueued(): records may have gone unread, the bound is unknown
    void resync(int device_seq) { seq_ = seen_ = device_seq; reset_bound(-1, 0); }

    // The record of step seen() + 1 was read.  Whether it asks for a verdict: never while `raised`, the reading call has one.
    bool absorb(const FrameScalars &r, const LedgerParams &p, bool raised)
    {
        const int s = ++seen_;
        last_ = r;
        live_at_build_ = r.live;
        const int64_t tasks_now = (int64_t)r.n_tasks2 + r.n_merged;       // ordinary tasks + packs of partial slices
        const bool two = interior_steps_.erase(s) != 0;                   // (in two passes: the record holds the second pass's count)
        tasks_last_ = two ? tasks_now * p.comp / std::max(1, p.comp_rest) : tasks_now;
        packs_last_ = two ? (int64_t)r.n_merged * p.comp / std::max(1, p.comp_rest) : r.n_merged;
        if (s > reset_step_) {           // (else: enqueued before an upload or a restore, whose particles it does not know)
            live_bound_ = std::min<int64_t>(p.slots_total, (int64_t)r.live + r.n_moves);   // births and arrivals <= moves
            bound_step_ = s;
            // ... and what was filled or injected after this step was enqueued (the record's live count does not include it)
            for (auto it = tally_.begin(); it != tally_.end();) {
                if (it->first < s) { it = tally_.erase(it); continue; }
                live_bound_ = std::min<int64_t>(p.slots_total, live_bound_ + it->second);
                ++it;
            }
        }
        processed_total_ += r.live;
        max_bucket_seen_ = std::max<int64_t>(max_bucket_seen_, r.max_bucket);
        if (p.world > 1 && r.xfer_cap_next > 0) cap_decisions_[s] = r.xfer_cap_next;
        return !raised && (p.world > 1 ? r.status_error != 0 : r.error != 0);
    }
    // the first verdict is kept until a call takes it (status 0: none)
    void hold_verdict(int status, const std::string &text) { if (status != 0 && pending_status_ == 0) { pending_status_ = status; pending_text_ = text; } }
    int pending_verdict() const { return pending_status_; }
    int take_verdict(std::string &text)
    {
        const int st = pending_status_;
        if (st != 0) { text = pending_text_; pending_status_ = 0; }
        return st;
    }

    // ---- hints for the launches to come ----
    // at most so many particles are alive at the NEXT build_grid (inside, < 0: unknown -- state was uploaded -- every owned
    // slot); rounded up to 64 Ki under graphs, so that a free-running population does not mean a capture per step
    int64_t alive_at_most(const LedgerParams &p, bool graphs) const
    {
        int64_t b = live_bound_ >= 0 ? live_bound_ : p.slots_total;
        for (int k = bound_step_; k < seq_ && b < p.slots_total; k++) b = (p.explosions ? 2 * b : b) + msg_room(p);
        b = std::min(b, p.slots_total);
        return graphs ? std::min<int64_t>((b + 65535) & ~(int64_t)65535, std::max<int64_t>(p.slots_total, 65536)) : b;
    }
    // size of the balanced force pass over `comp_pass` cells: the tasks of the last step read, else the bound of the live
    // count (a pass over part of the cells gets its share).  High word: about how many packs of partly filled slices the
    // pass will have, in steps of 64 so that the launch shape does not change with every step.
    int64_t pairs_hint(const LedgerParams &p, int comp_pass) const
    {
        const int64_t tasks = (seen_ > 0 && tasks_last_ > 0) ? tasks_last_ : (live_bound_ >= 0 ? live_bound_ : p.slots_total) / 64 + p.comp;
        const int64_t packs = ((seen_ > 0 ? packs_last_ : 0) + 63) & ~(int64_t)63;
        return (tasks * comp_pass / std::max(1, p.comp)) | ((packs * comp_pass / std::max(1, p.comp)) << 32);
    }
    // arrivals on top of the own particles: about what the op lists and move records of a step hold at most
    static int64_t lifecycle_bound(const LedgerParams &p, int64_t bound) { return bound + msg_room(p) + p.kill_room; }
    // which instance replays the lists (2048 / 4096 / bucket_max operations sorted in LDS): by the longest list of the last
    // step read; and as bits of a captured graph's key
    int bucket_cap(const LedgerParams &p) const { const int n = seen_ > 0 ? last_.max_bucket : 0; return n > 4096 ? p.bucket_max : n > 2048 ? 4096 : 2048; }
    uint64_t bucket_key(const LedgerParams &p) const { const int cap = bucket_cap(p); return cap > 4096 ? 2ull << 61 : cap > 2048 ? 1ull << 61 : 0ull; }
    bool big_cells() const { return seen_ > 0 && last_.max_cell_raw > 960; }     // is a cell with more than 1024 ids to be expected?
    // the transfer capacity in force from the step about to be built, s = seq() + 1: the decisions of steps <= s - 2
    int adopt_cap(const LedgerParams &p)
    {
        int cap = p.xfer_cap;
        for (auto it = cap_decisions_.begin(); it != cap_decisions_.end() && it->first <= seq_ - 1; it = cap_decisions_.erase(it)) cap = it->second;
        return std::max(p.xfer_cap0, std::min(cap, p.xfer_cap_max));
    }

    // ---- what the other units did ----
    // every particle placed counts, also when the record of a step enqueued before the call is read later: tallied under
    // the last step enqueued until the record of the step after it -- the first that counts them -- has been read
    void filled(int64_t placed)                  // (what was placed found a free slot: no more than the slots)
    {
        if (live_bound_ >= 0) live_bound_ += placed;
        tally_[seq_] += placed;
    }
    void injected(const LedgerParams &p, int64_t max_count)      // (every entry may be placed, or none)
    {
        if (live_bound_ >= 0) live_bound_ = std::min(p.slots_total, live_bound_ + max_count);
        tally_[seq_] += max_count;
    }
    void uploaded() { reset_bound(-1, 0); }
    // the snapshot holds the particles of this moment: the bound and the steps whose growth alive_at_most() adds to it now,
    // which it adds again after the restore
    void snapshot_saved() { snapshot_live_bound_ = live_bound_; snapshot_growth_steps_ = seq_ - bound_step_; }
    void snapshot_restored() { reset_bound(snapshot_live_bound_, snapshot_growth_steps_); }
    void frame_live(int live) { live_at_build_ = live; }       // read from the device's own record inside a frame

    // ---- for the getters ----
    const FrameScalars &last() const { return last_; }          // the record of the last step read
    int last_live() const { return live_at_build_; }            // its live count (-1: none yet)
    int64_t particles_processed() const { return processed_total_; }    // sum over the steps read of the live particles at build_grid
    int64_t longest_list() const { return max_bucket_seen_; }

private:
    static int64_t msg_room(const LedgerParams &p) { return 2 * (int64_t)p.xfer_cap + 2 * (int64_t)p.xfer2_cap + (int64_t)p.far_cap * p.world; }
    // The particles were replaced behind the last step enqueued: `bound` of them at most (-1: unknown) before the growth of
    // `growth_steps` steps.  The records of the steps enqueued so far do not know them and what was tallied for those
    // records went with the particles it counted.
    void reset_bound(int64_t bound, int growth_steps)
    {
        live_bound_ = bound;
        reset_step_ = seq_;
        bound_step_ = seq_ - growth_steps;
        tally_.clear();
    }

    int seq_ = 0, seen_ = 0, run_ahead_ = 1;
    FrameScalars last_{};
    int live_at_build_ = -1;
    bool interior_ran_ = false;
    std::set<int> interior_steps_;           // the steps in two passes whose records have not been read yet
    int64_t tasks_last_ = 0, packs_last_ = 0;    // force tasks of the last step read (all passes); of which packs of partly filled slices
    int64_t live_bound_ = 0, snapshot_live_bound_ = 0;     // live particles once step bound_step_ has run, at most (-1: unknown)
    int bound_step_ = 0;                     // ... the steps after it are the ones alive_at_most() adds the growth of
    int snapshot_growth_steps_ = 0;          // ... of the saved bound: seq() - bound_step_ at the save
    int reset_step_ = 0;                    // the last step enqueued before the particles were last replaced (upload, restore)
    std::map<int, int64_t> tally_;           // step k -> particles the fills and injects enqueued after it placed at most
    std::map<int, int> cap_decisions_;       // step -> the transfer capacity all ranks agreed on in it
    int64_t processed_total_ = 0, max_bucket_seen_ = 0;
    int pending_status_ = 0;                 // the held verdict and its text
    std::string pending_text_;
};

}  // namespace psamd
