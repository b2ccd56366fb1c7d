// ring_routes.hpp -- the message routes of the slab ring and the buffers behind them, stated once (part of
// ps_ring_rccl.cpp, which alone includes it).  Nothing here touches the GPU or RCCL.
//
// Message routes (particlesystem_amd/slab.py::routes() says the same in Python, and tests/test_host_ring_cpu.py holds
// the two against each other through --routes): after slab_build the halo snapshots (rank r's halo_out[above] ->
// rank r+1's halo_in[below]; halo_out[below] -> rank r-1's halo_in[above]); after slab_pairs the force records of lent
// layers (force_out -> rank r-1's force_in); after slab_apply the particles that change owner, on the ring
// (xfer_out[below] -> rank (r-1)%W's xfer_in[above], xfer_out[above] -> rank (r+1)%W's xfer_in[below]; hop two
// likewise in worlds of four or more).  The status records, the snapshot blocks of an all-pairs run (or the cell sums of a far-field run, in the same buffers) and the far
// outboxes are all-gathered.  All sizes are fixed by the plan; a message of 0 bytes does not exist.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "psamd.h"

namespace {

enum Phase { HALO, FORCE, XFER };
// message slots: the `which` numbering of psamd_slab_msg_download (include/psamd.h), the one the library's message table
// and slab.py use; in a pair + BELOW / ABOVE
enum Slot { HALO_OUT = 0, HALO_IN = 2, FORCE_OUT = 4, FORCE_IN = 5, XFER_OUT = 6, XFER_IN = 8, STATUS_OUT = 10, STATUS_IN = 11,
            ALLG_OUT = 12, ALLG_IN = 13, XFER2_OUT = 14, XFER2_IN = 16, FAR_OUT = 18, FAR_IN = 19, NUM_SLOTS = 20 };
enum { BELOW = 0, ABOVE = 1 };
const char *const kPhaseName[3] = {"halo", "force", "xfer"};
const char *const kSlotName[NUM_SLOTS] = {"halo_out[below]", "halo_out[above]", "halo_in[below]", "halo_in[above]", "force_out", "force_in",
                                          "xfer_out[below]", "xfer_out[above]", "xfer_in[below]", "xfer_in[above]", "status_out", "status_in", "allg_out", "allg_in",
                                          "xfer2_out[below]", "xfer2_out[above]", "xfer2_in[below]", "xfer2_in[above]", "far_out", "far_in"};

// dir: 0 travels down the ring, 1 up; hop: 1 to a ring neighbour, 2 to the rank beyond it
struct Route { Phase phase; int out_slot, peer, in_slot, dir, hop; };

// Every message `rank` of `world` may send.  Which of them exist is decided by the sizes alone (0 bytes: no such message).
std::vector<Route> routes(int rank, int world)
{
    std::vector<Route> v;
    if (rank > 0) {
        v.push_back({HALO, HALO_OUT + BELOW, rank - 1, HALO_IN + ABOVE, 0, 1});
        v.push_back({FORCE, FORCE_OUT, rank - 1, FORCE_IN, 0, 1});
    }
    if (rank + 1 < world) v.push_back({HALO, HALO_OUT + ABOVE, rank + 1, HALO_IN + BELOW, 1, 1});
    // the ring: hop one in worlds of two or more, hop two (a two-layer jump over a rank whose state is one layer) of four or more
    for (int hop = 1; hop <= 2 && world >= 2 * hop; hop++) {
        const int out = hop == 1 ? XFER_OUT : XFER2_OUT, in = hop == 1 ? XFER_IN : XFER2_IN;
        v.push_back({XFER, out + BELOW, (rank - hop + world) % world, in + ABOVE, 0, hop});
        v.push_back({XFER, out + ABOVE, (rank + hop) % world, in + BELOW, 1, hop});
    }
    return v;
}

// What `rank` may receive: the other ranks' routes that end here, seen from this side (peer = the sender).
std::vector<Route> receives(int rank, int world)
{
    std::vector<Route> v;
    for (int from = 0; from < world; from++)
        for (Route m : routes(from, world))
            if (from != rank && m.peer == rank) { m.peer = from; v.push_back(m); }
    return v;
}

// A slot's buffer.  (An all-gathered in-buffer holds `world` blocks of the size given here.)
struct Buf { void *p; int64_t bytes; };
Buf buf_of(const psamd_slab_buffers &b, int slot)
{
    const int k = slot & 1;
    switch (slot & ~1) {
    case HALO_OUT: return {b.halo_out[k], b.halo_out_bytes[k]};
    case HALO_IN: return {b.halo_in[k], b.halo_in_bytes[k]};
    case FORCE_OUT: return k ? Buf{b.force_in, b.force_in_bytes} : Buf{b.force_out, b.force_out_bytes};
    case XFER_OUT: return {b.xfer_out[k], b.xfer_bytes};
    case XFER_IN: return {b.xfer_in[k], b.xfer_bytes};
    case STATUS_OUT: return {k ? b.status_in : b.status_out, b.status_bytes};
    case ALLG_OUT: return {k ? b.allg_in : b.allg_out, b.allg_bytes};
    case XFER2_OUT: return {b.xfer2_out[k], b.xfer2_bytes};
    case XFER2_IN: return {b.xfer2_in[k], b.xfer2_bytes};
    case FAR_OUT: return {k ? b.far_in : b.far_out, b.far_bytes};
    }
    return {nullptr, 0};
}

// Both ends of every message must agree on its size BEFORE the first step: RCCL matches a send and a receive by order
// alone, and two neighbours that disagree (different halo_cap_cell / xfer_cap / plans) would sit in the transfer until the
// watchdog ends them.  Every rank's sizes, by slot, are checked against the routes: the sender's out-slot against the
// receiver's in-slot; an all-gathered buffer has one size everywhere.
struct SizeTable { int64_t bytes[NUM_SLOTS]; };
SizeTable sizes_of(const psamd_slab_buffers &b)
{
    SizeTable t{};
    for (int slot = 0; slot < NUM_SLOTS; slot++) t.bytes[slot] = buf_of(b, slot).bytes;
    return t;
}
int sizes_agree(const std::vector<SizeTable> &all)
{
    const int W = (int)all.size();
    auto differ = [&](int a, int out_slot, int b, int in_slot) {
        const long long x = all[(size_t)a].bytes[out_slot], y = all[(size_t)b].bytes[in_slot];
        if (x != y) std::fprintf(stderr, "message sizes disagree: %s of rank %d is %lld bytes, %s of rank %d expects %lld (same halo_cap_cell / xfer_cap / cuts on every rank?)\n",
                                 kSlotName[out_slot], a, x, kSlotName[in_slot], b, y);
        return x != y;
    };
    for (int r = 0; r < W; r++) {
        for (const Route &m : routes(r, W)) if (differ(r, m.out_slot, m.peer, m.in_slot)) return 1;
        for (int slot : {STATUS_OUT, ALLG_OUT, FAR_OUT}) if (differ(r, slot, 0, slot)) return 1;
    }
    return 0;
}

}  // namespace
