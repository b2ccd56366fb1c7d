// Walks csrc/step_ledger.hpp for tests/test_step_ledger_cpu.py: reads scripts of operations on stdin and prints what the
// ledger lets the rest of the host see after every one.  The few lines of step.hip around the ledger (consume_scalars,
// finish_step, drain_scalars, the adoption in slab_build) are restated here over two records in plain memory in place
// of the pinned pair; a record's verdict is its error word.  Host only; the test builds it with the address and
// undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "step_ledger.hpp"

using namespace psamd;

struct Host {
    StepLedger L;
    LedgerParams p{};
    FrameScalars h_fs[2]{};     // the two records a step's number picks from
    std::string err;
    int most_unread = 0;
};

static void consume(Host &h, int upto)
{
    int verdict = 0;
    while (h.L.seen() < h.L.seq()) {
        const int s = h.L.seen() + 1;
        if (h.h_fs[s & 1].seq != s) {
            if (s > upto) break;
            std::printf("STALL %d\n", s);       // (a script must let the records it waits for arrive first)
            std::exit(2);
        }
        const FrameScalars r = h.h_fs[s & 1];
        if (h.L.absorb(r, h.p, verdict != 0)) { verdict = h.p.world > 1 ? r.status_error : r.error; h.err = "step-" + std::to_string(s); }
    }
    h.L.hold_verdict(verdict, h.err);
}

static void show(const Host &h, int ret)
{
    const StepLedger &L = h.L;
    const LedgerParams &p = h.p;
    const int64_t bg = L.alive_at_most(p, true), bn = L.alive_at_most(p, false);
    std::printf("seq=%d seen=%d bound=%lld/%lld", L.seq(), L.seen(), (long long)bg, (long long)bn);
    const int comp[3] = {p.comp, p.comp_int, p.comp_rest};
    const char *const name[3] = {"hint", "hint_int", "hint_rest"};
    for (int k = 0; k < 3; k++) {
        const int64_t v = L.pairs_hint(p, comp[k]);
        std::printf(" %s=%lld/%lld", name[k], (long long)(v & 0xffffffffll), (long long)(v >> 32));
    }
    std::printf(" life=%lld/%lld bucket=%d/%llu big=%d cap=%d live=%d gridmax=%d/%d processed=%lld longest=%lld pending=%d ret=%d err=%s unread=%d\n",
                (long long)StepLedger::lifecycle_bound(p, bg), (long long)StepLedger::lifecycle_bound(p, bn), L.bucket_cap(p),
                (unsigned long long)(L.bucket_key(p) >> 61), (int)L.big_cells(), p.xfer_cap, L.last_live(), L.last().gridmax[0], L.last().gridmax[1],
                (long long)L.particles_processed(), (long long)L.longest_list(), L.pending_verdict(), ret, h.err.empty() ? "-" : h.err.c_str(), h.most_unread);
}

int main()
{
    Host h;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op)) continue;
        long long a = 0;
        int ret = 0;
        if (op == "cfg") {
            h = Host{};
            int expl = 0, ra = 1;
            long long slots = 0;
            LedgerParams &p = h.p;
            in >> p.world >> expl >> ra >> slots >> p.xfer_cap >> p.xfer2_cap >> p.far_cap >> p.xfer_cap0 >> p.xfer_cap_max >> p.comp >> p.comp_int >> p.comp_rest;
            p.slots_total = slots; p.explosions = expl != 0;
            p.kill_room = p.world > 1 ? (int64_t)p.world * 4080 : 0; p.bucket_max = 8192;
            h.L.set_run_ahead(ra);
        } else if (op == "step") {              // finish_step; with 1, slab_pairs_interior ran its pass in this frame
            in >> a;
            if (a) h.L.interior_pass_ran();
            h.L.enqueued();
            h.most_unread = std::max(h.most_unread, h.L.seq() - h.L.seen());
            consume(h, h.L.due());
            ret = h.L.take_verdict(h.err);
        } else if (op == "rec") {               // the device publishes a step's record
            FrameScalars r{};
            in >> r.seq >> r.live >> r.n_moves >> r.n_tasks2 >> r.n_merged >> r.max_bucket >> r.max_cell_raw >> r.xfer_cap_next >> r.error >> r.status_error >> r.gridmax[0] >> r.gridmax[1];
            h.h_fs[r.seq & 1] = r;
        } else if (op == "read") { in >> a; consume(h, (int)a); }
        else if (op == "drainq") consume(h, h.L.seq());
        else if (op == "drain") { consume(h, h.L.seq()); ret = h.L.take_verdict(h.err); }
        else if (op == "fill") { in >> a; h.L.filled(a); }
        else if (op == "upload") h.L.uploaded();
        else if (op == "inject") { in >> a; h.L.injected(h.p, a); }
        else if (op == "save") h.L.snapshot_saved();
        else if (op == "restore") h.L.snapshot_restored();
        else if (op == "resync") { in >> a; h.L.resync((int)a); }
        else if (op == "build") h.p.xfer_cap = h.L.adopt_cap(h.p);      // slab_build of step seq + 1
        else if (op == "ra") { in >> a; h.L.set_run_ahead((int)a); }
        else if (op == "framelive") { in >> a; h.L.frame_live((int)a); }
        else { std::printf("BAD %s\n", op.c_str()); return 2; }
        show(h, ret);
    }
    return 0;
}
