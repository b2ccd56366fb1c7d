"""The ledger of steps (csrc/step_ledger.hpp) against the loose fields of the context it replaced, without a GPU.

step_ledger_dump.cpp -- a stand-alone program, built with the address and undefined-behaviour sanitizers -- reads scripts
of operations and prints, after every one, all the ledger lets the host see.  `Old` below holds the fields the context
had before (scalars_seq, scalars_seen, last, live_bound, the tally, cap_decisions, pending_status ...) with the
statements of step.hip, io.hip and services.hip that read and wrote them, one for one; both sides take the same
scripts and every printed field is compared after every operation.  Where the ledger's rules have changed since (the live
bound across fill, upload and restore) `Old` was changed with them, line for line: it says HOW the ledger computes, and
would agree with it on a rule that is wrong.  WHETHER the live bound is a bound is checked against `World`, the particles
themselves (the live_bound tests): the bound a step is sized from is never below the particles alive at its build.

A script is what a host does to one context: `step` is finish_step (the step is enqueued, the records due are read, the
verdict is returned), `rec` the device publishing a step's record into one of the two host records, `read U` a bare
consume_scalars(U), `drainq` / `drain` drain_scalars (quiet / reporting), `build` slab_build's adoption of the transfer
capacity; the rest are the other units' calls.  A record's verdict is its error word, its text the step's number."""
import os
import random
import shutil
import subprocess
from types import SimpleNamespace

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "particlesystem_amd", "csrc")
STATUS_KILL_CAP, BUCKET_MAX = 4080, 8192
REC_FIELDS = ("seq", "live", "n_moves", "n_tasks2", "n_merged", "max_bucket", "max_cell_raw", "xfer_cap_next", "error", "status_error", "gm0", "gm1")


def record(seq, live=0, n_moves=0, n_tasks2=0, n_merged=0, max_bucket=0, max_cell_raw=0, xfer_cap_next=0, error=0, status_error=0, gm0=0, gm1=0):
    return SimpleNamespace(**{k: v for k, v in locals().items()})


def rec_line(r):
    return "rec " + " ".join(str(getattr(r, k)) for k in REC_FIELDS)


def config(world=1, expl=0, ra=1, slots=100000, xfer=0, xfer2=0, far=0, cap0=0, capmax=0, comp=512, comp_int=0, comp_rest=0):
    return SimpleNamespace(**{k: v for k, v in locals().items()})


def cfg_line(g):
    return "cfg %d %d %d %d %d %d %d %d %d %d %d %d" % (g.world, g.expl, g.ra, g.slots, g.xfer, g.xfer2, g.far, g.cap0, g.capmax, g.comp, g.comp_int, g.comp_rest)


class Old:
    """the context's fields and the statements over them (c-> is self., c->P. is self.P.), kept in step with the ledger's rules"""

    def __init__(self, g):
        self.P = SimpleNamespace(world=g.world, explosions=bool(g.expl), slots_total=g.slots, xfer_cap=g.xfer, xfer2_cap=g.xfer2, far_cap=g.far,
                                 xfer_cap0=g.cap0, xfer_cap_max=g.capmax)
        self.comp, self.comp_int, self.comp_rest = g.comp, g.comp_int, g.comp_rest       # comp_count(P), (P_int), (P_rest)
        self.h_fs = [record(0), record(0)]
        self.scalars_seq = self.scalars_seen = 0
        self.run_ahead = g.ra
        self.last = record(0)
        self.live_at_build = -1
        self.interior_ran = False
        self.interior_steps = set()
        self.tasks_last = self.packs_last = 0
        self.live_bound = self.snapshot_live_bound = 0
        self.bound_step = self.reset_step = self.snapshot_growth_steps = 0
        self.tally = {}
        self.cap_decisions = {}
        self.processed_total = self.max_bucket_seen = 0
        self.bucket_cap0 = 2048
        self.pending_status, self.pending_err = 0, ""
        self.err = ""
        self.most_unread = 0

    # ---- step.hip ----
    def check_device_errors(self, s, r):
        self.err = "step-%d" % s
        return r.status_error if self.P.world > 1 else r.error

    def consume_scalars(self, upto):
        verdict = 0
        while self.scalars_seen < self.scalars_seq:
            s = self.scalars_seen + 1
            if s <= upto:
                assert self.h_fs[s & 1].seq == s, "the script waits for a record that never arrives"     # wait_scalars
            elif self.h_fs[s & 1].seq != s:
                break
            r = self.h_fs[s & 1]
            self.scalars_seen = s
            self.last = r
            self.live_at_build = r.live
            tasks_now = r.n_tasks2 + r.n_merged
            two = s in self.interior_steps
            self.interior_steps.discard(s)
            self.tasks_last = tasks_now * self.comp // max(1, self.comp_rest) if two else tasks_now
            self.packs_last = r.n_merged * self.comp // max(1, self.comp_rest) if two else r.n_merged
            if s > self.reset_step:
                self.live_bound = min(self.P.slots_total, r.live + r.n_moves)
                self.bound_step = s
                for k in sorted(self.tally):
                    if k < s:
                        del self.tally[k]
                        continue
                    self.live_bound = min(self.P.slots_total, self.live_bound + self.tally[k])
            self.processed_total += r.live
            self.max_bucket_seen = max(self.max_bucket_seen, r.max_bucket)
            if self.P.world > 1 and r.xfer_cap_next > 0:
                self.cap_decisions[s] = r.xfer_cap_next
            if verdict == 0 and (r.status_error != 0 if self.P.world > 1 else r.error != 0):
                verdict = self.check_device_errors(s, r)
        if verdict != 0 and self.pending_status == 0:
            self.pending_status, self.pending_err = verdict, self.err

    def take_verdict(self):
        if self.pending_status == 0:
            return 0
        st = self.pending_status
        self.err = self.pending_err
        self.pending_status = 0
        return st

    def finish_step(self):
        self.scalars_seq += 1
        seq = self.scalars_seq
        if self.interior_ran:
            self.interior_steps.add(seq)
        self.interior_ran = False
        self.most_unread = max(self.most_unread, self.scalars_seq - self.scalars_seen)
        self.consume_scalars(seq - 1 if self.run_ahead else seq)
        return self.take_verdict()

    def drain_scalars(self, quiet):
        self.consume_scalars(self.scalars_seq)
        return 0 if quiet else self.take_verdict()

    def live_bound_of(self, graphs):
        P = self.P
        b = self.live_bound if self.live_bound >= 0 else P.slots_total
        k = self.bound_step
        while k < self.scalars_seq and b < P.slots_total:
            if P.explosions:
                b *= 2
            b += 2 * P.xfer_cap + 2 * P.xfer2_cap + P.far_cap * P.world
            k += 1
        b = min(b, P.slots_total)
        return min((b + 65535) & ~65535, max(P.slots_total, 65536)) if graphs else b

    def pairs_hint(self, comp_pass):
        if self.scalars_seen > 0 and self.tasks_last > 0:
            tasks_hint = self.tasks_last
        else:
            tasks_hint = (self.live_bound if self.live_bound >= 0 else self.P.slots_total) // 64 + self.comp
        packs = ((self.packs_last if self.scalars_seen > 0 else 0) + 63) & ~63
        return tasks_hint * comp_pass // max(1, self.comp), packs * comp_pass // max(1, self.comp)

    def lifecycle_bound(self, bound):
        P = self.P
        return bound + 2 * P.xfer_cap + 2 * P.xfer2_cap + P.far_cap * P.world + (P.world * STATUS_KILL_CAP if P.world > 1 else 0)

    def pick_bucket_cap(self):
        last = self.last.max_bucket if self.scalars_seen > 0 else 0
        self.bucket_cap0 = BUCKET_MAX if last > 4096 else 4096 if last > 2048 else 2048
        return 2 if self.bucket_cap0 > 4096 else 1 if self.bucket_cap0 > 2048 else 0          # (<< 61)

    def big_cells_hint(self):
        return self.scalars_seen > 0 and self.last.max_cell_raw > 960

    def slab_build(self):
        P = self.P
        s = self.scalars_seq + 1
        cap = P.xfer_cap
        for k in sorted(self.cap_decisions):
            if k > s - 2:
                break
            cap = self.cap_decisions.pop(k)
        cap = max(P.xfer_cap0, min(cap, P.xfer_cap_max))
        if cap != P.xfer_cap:
            P.xfer_cap = cap

    def resync_scalars(self, device_seq):
        self.scalars_seq = self.scalars_seen = device_seq
        self.reset_bound(-1, 0)

    def reset_bound(self, bound, growth_steps):
        self.live_bound = bound
        self.reset_step = self.scalars_seq
        self.bound_step = self.scalars_seq - growth_steps
        self.tally.clear()

    # ---- io.hip, services.hip ----
    def fill_particles(self, placed):
        if self.live_bound >= 0:
            self.live_bound += placed
        self.tally[self.scalars_seq] = self.tally.get(self.scalars_seq, 0) + placed

    def upload_particles(self):
        self.reset_bound(-1, 0)

    def inject(self, max_count):
        if self.live_bound >= 0:
            self.live_bound = min(self.P.slots_total, self.live_bound + max_count)
        self.tally[self.scalars_seq] = self.tally.get(self.scalars_seq, 0) + max_count

    def snapshot_save(self):
        self.snapshot_live_bound = self.live_bound
        self.snapshot_growth_steps = self.scalars_seq - self.bound_step

    def snapshot_restore(self):
        self.reset_bound(self.snapshot_live_bound, self.snapshot_growth_steps)

    # ---- a script's line, and what the program prints after it ----
    def run(self, line):
        op, *args = line.split()
        a = [int(v) for v in args]
        ret = 0
        if op == "step":
            if a[0]:
                self.interior_ran = True          # slab_pairs_interior
            ret = self.finish_step()
        elif op == "rec":
            r = record(*a)
            self.h_fs[r.seq & 1] = r
        elif op == "read":
            self.consume_scalars(a[0])
        elif op == "drainq":
            ret = self.drain_scalars(True)
        elif op == "drain":
            ret = self.drain_scalars(False)
        elif op == "fill":
            self.fill_particles(a[0])
        elif op == "upload":
            self.upload_particles()
        elif op == "inject":
            self.inject(a[0])
        elif op == "save":
            self.snapshot_save()
        elif op == "restore":
            self.snapshot_restore()
        elif op == "resync":
            self.resync_scalars(a[0])
        elif op == "build":
            self.slab_build()
        elif op == "ra":
            self.run_ahead = a[0]                 # psamd_set_run_ahead
        elif op == "framelive":
            self.live_at_build = a[0]             # psamd_get_gridmax inside a frame
        else:
            raise AssertionError(op)
        bg, bn = self.live_bound_of(True), self.live_bound_of(False)
        key = self.pick_bucket_cap()
        hints = " ".join("%s=%d/%d" % ((name,) + self.pairs_hint(k)) for name, k in (("hint", self.comp), ("hint_int", self.comp_int), ("hint_rest", self.comp_rest)))
        return ("seq=%d seen=%d bound=%d/%d %s life=%d/%d bucket=%d/%d big=%d cap=%d live=%d gridmax=%d/%d processed=%d longest=%d pending=%d ret=%d err=%s unread=%d"
                % (self.scalars_seq, self.scalars_seen, bg, bn, hints, self.lifecycle_bound(bg), self.lifecycle_bound(bn), self.bucket_cap0, key,
                   self.big_cells_hint(), self.P.xfer_cap, self.live_at_build, self.last.gm0, self.last.gm1, self.processed_total, self.max_bucket_seen,
                   self.pending_status, ret, self.err or "-", self.most_unread))


@pytest.fixture(scope="module")
def ledger(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path_factory.mktemp("step_ledger") / "step_ledger_dump")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "step_ledger_dump.cpp"), "-o", exe], check=True)

    def walk(g, lines):
        """both sides over one script: the program's lines (equal to the restatement's), as dicts"""
        out = subprocess.run([exe], input="\n".join([cfg_line(g)] + lines) + "\n", check=True, capture_output=True, text=True)
        assert out.stderr == ""
        new = out.stdout.splitlines()
        old = Old(g)
        want = [old.run("ra %d" % g.ra)] + [old.run(line) for line in lines]        # (the cfg line prints the fresh state)
        assert len(new) == len(want)
        for k, (n, w) in enumerate(zip(new, want)):
            assert n == w, "after line %d (%s)" % (k, ([cfg_line(g)] + lines)[k])
        return [dict(f.split("=", 1) for f in n.split(" ")) for n in new[1:]]
    walk.exe = exe
    return walk


# ---- fixed-seed random scripts ----
def random_script(rng, g, n_ops=60, world=None):
    """A host's calls in any order a host may make them, and the device publishing records in order: early (as soon as
    the step is enqueued), on time (just before the call that waits for it) or late (after a call peeked and missed it).
    With a `world` (World below) the calls act on its particles too and the records are the ones its steps wrote."""
    lines, seq, seen, arrived, ra = [], 0, 0, 0, g.ra       # arrived: the last record the device has published

    def publish(upto):
        nonlocal arrived
        while arrived < upto:
            arrived += 1
            if world:
                lines.append(rec_line(world.records.pop(arrived)))
                continue
            err = rng.choice((0, 0, 0, 0, 0, 64, 512))
            lines.append(rec_line(record(arrived, live=rng.randrange(0, g.slots), n_moves=rng.randrange(0, 3000),
                                         n_tasks2=rng.choice((0, rng.randrange(1, 9000))), n_merged=rng.randrange(0, 700),
                                         max_bucket=rng.choice((0, 100, 2048, 2049, 4096, 4097, 9000)), max_cell_raw=rng.choice((0, 960, 961, 5000)),
                                         xfer_cap_next=rng.choice((0, 0, 1, 500, 4000, 100000)), error=err if rng.random() < 0.5 else 0,
                                         status_error=err if rng.random() < 0.5 else 0, gm0=rng.randrange(0, 300), gm1=rng.randrange(0, 200))))

    def read(upto):                                 # consume_scalars(upto): the records it waits for must be there; it reads all that are
        nonlocal seen
        publish(min(upto, seq))
        seen = max(seen, min(arrived, seq))

    while len(lines) < n_ops:
        op = rng.choice(("step",) * 8 + ("rec",) * 4 + ("read", "drainq", "drain", "fill", "upload", "inject", "inject", "save", "restore", "build", "build",
                                                        "resync", "ra", "framelive"))
        if world and not world.call(op, lines):
            continue                                # (the call and its amount are the world's, or the world has no such call)
        if op == "step":
            if g.world > 1 and rng.random() < 0.5:
                lines.append("build")
            seq += 1
            if world:
                world.step(seq)                     # (the bound this step is sized from is the one after the line before)
            if rng.random() < 0.3:
                publish(seq)                        # (the step's launches are out before the host books it)
            read(seq - 1 if ra else seq)
            lines.append("step %d" % (g.comp_int > 0 and rng.random() < 0.4))
        elif op == "rec":
            if arrived < seq:
                publish(arrived + 1)
        elif op == "read":
            upto = rng.randrange(0, seq + 2)
            read(upto)
            lines.append("read %d" % upto)
        elif op in ("drainq", "drain"):
            read(seq)
            lines.append(op)
        elif op in ("fill", "inject"):
            lines.append("%s %d" % (op, rng.choice((0, 1, 777, g.slots))))
        elif op == "resync":
            if rng.random() < 0.2:                  # (rare: a failed launch; the device's count is what it has published)
                seq = seen = arrived
                lines.append("resync %d" % arrived)
        elif op == "ra":
            if rng.random() < 0.2:
                ra = 1 - ra
                lines.append("ra %d" % ra)
        elif op == "framelive":
            lines.append("framelive %d" % rng.randrange(0, g.slots))
        else:
            lines.append(op)
    return lines


def random_config(rng, k):
    world = 1 + (k & 1)
    slots = rng.choice((5000, 70000, 300000))
    cap0 = rng.choice((16, 256)) if world > 1 else 0
    comp = rng.choice((64, 512, 1000))
    comp_int = rng.choice((0, comp // 3)) if world > 1 else 0
    return config(world=world, expl=(k >> 1) & 1, ra=(k >> 2) & 1, slots=slots, xfer=cap0, xfer2=rng.choice((0, 8)) if world > 1 else 0,
                  far=rng.choice((0, 4)) if world > 1 else 0, cap0=cap0, capmax=cap0 * rng.choice((1, 8, 64)), comp=comp, comp_int=comp_int,
                  comp_rest=comp - comp_int if comp_int else 0)


def test_random_scripts_leave_every_field_equal(ledger):
    """240 scripts of 60 lines: worlds 1 and 2, explosions, run-ahead 0 and 1 (and switched under way); the live bound is
    printed with graphs on and off.  Never more than two records are unread."""
    met = set()
    for k in range(240):
        rng = random.Random(9000 + k)
        g = random_config(rng, k)
        met.add((g.world, g.expl, g.ra))
        lines = random_script(rng, g)
        states = ledger(g, lines)
        assert all(int(s["unread"]) <= 2 for s in states)
    assert len(met) == 8


# ---- the live bound against the particles themselves ----
class World:
    """The truth beside a script: `pop`, the particles alive, by the rules of the device and not of the ledger.
      step     pop becomes anything in [0, min(slots, (2 pop if explosions else pop) + room)]: a child per particle at most,
               and the messages' room (StepLedger::msg_room, restated from the config: the records carry no capacity
               decision, so the capacity stays the config's); the step's record holds pop at its build and any
               n_moves >= the growth
      fill n   + n, inject n: + anything in [0, n]; both stop at `slots`
      upload   anything in [0, slots];  save / restore: store pop / put it back
    `at_build` lists pop at every step's build, in the order of the script's step lines."""

    def __init__(self, rng, g):
        self.rng, self.g = rng, g
        self.room = 2 * g.xfer + 2 * g.xfer2 + g.far * g.world
        self.pop, self.saved = 0, None
        self.at_build, self.records = [], {}

    def step(self, s):
        rng, g, before = self.rng, self.g, self.pop
        top = min(g.slots, (2 * before if g.expl else before) + self.room)
        self.pop = rng.choice((top, top, before, before, before // 2, rng.randint(0, top), rng.randint(0, top)))
        self.at_build.append(before)
        self.records[s] = record(s, live=before, n_moves=max(0, self.pop - before) + rng.choice((0, 0, rng.randrange(0, 40))),
                                 n_tasks2=rng.choice((0, rng.randrange(1, 9000))), n_merged=rng.randrange(0, 700),
                                 max_bucket=rng.choice((0, 100, 2049, 4097)), max_cell_raw=rng.choice((0, 961)))

    def call(self, op, lines):
        """a call that changes the particles: its line, with an amount of the world's choosing (False: done here, or
        not a call of this world -- resync, a failed launch, leaves the particles in no state the rules describe)"""
        rng, g = self.rng, self.g
        if op in ("fill", "inject"):
            n = rng.choice((0, 1, 777, g.slots // 3, g.slots // 2, g.slots))
            self.pop = min(g.slots, self.pop + (n if op == "fill" else rng.choice((0, n, rng.randint(0, n)))))
            lines.append("%s %d" % (op, n))
        elif op == "upload":
            self.pop = rng.choice((g.slots, g.slots // 2, rng.randint(0, g.slots), rng.randint(0, 100)))
            lines.append(op)
        elif op == "save":
            self.saved = self.pop
            lines.append(op)
        elif op == "restore":
            if self.saved is not None:              # (psamd_snapshot_restore without a snapshot is refused before the ledger hears of it)
                self.pop = self.saved
                lines.append(op)
        else:
            return op != "resync"
        return False


def bound_shortfalls(states, lines, at_build):
    """[(line number, bound, pop)] for every step whose bound -- the one printed after the line before it, graphs off or
    on -- was below the particles alive at its build"""
    steps = [k for k, line in enumerate(lines) if line.startswith("step")]
    assert len(steps) == len(at_build)
    short = []
    for k, pop in zip(steps, at_build):
        bg, bn = (int(v) for v in states[k - 1]["bound"].split("/")) if k else (0, 0)       # (a fresh ledger: 0 of 0 particles)
        if min(bg, bn) < pop:
            short.append((k, min(bg, bn), pop))
    return short


def hand_script(*items):
    """(lines, pop at the build of every step): a step is written ("step 0", pop at its build)"""
    return [i if isinstance(i, str) else i[0] for i in items], [i[1] for i in items if not isinstance(i, str)]


# a call that changes the particles while a record from before it is unread: what the record says no longer holds
HAND_SCRIPTS = {
    # the record of step 1 (1000 alive, 10 moves) is read by the call that enqueues step 2, after the upload of 50 000
    "upload": (config(ra=1), hand_script("fill 1000", ("step 0", 1000), rec_line(record(1, live=1000, n_moves=10)), "upload", ("step 0", 50000),
                                         rec_line(record(2, live=50000)), ("step 0", 50000))),
    "fill": (config(ra=1), hand_script("fill 1000", ("step 0", 1000), rec_line(record(1, live=1000, n_moves=10)), "fill 49000", ("step 0", 50000),
                                       rec_line(record(2, live=50000)), ("step 0", 50000))),
    # 50 000 saved, the context brought down to 1000 and stepped, the snapshot put back with that step's record unread
    "restore": (config(ra=1), hand_script("fill 50000", "save", "upload", ("step 0", 1000), rec_line(record(1, live=1000)), "restore", ("step 0", 50000),
                                          rec_line(record(2, live=50000)), ("step 0", 50000))),
    # explosions: step 1 doubles 1000 to 2000 and its record is unread at the save; everything is read before the restore
    "save": (config(ra=1, expl=1), hand_script("fill 1000", ("step 0", 1000), "save", rec_line(record(1, live=1000, n_moves=1000)), "drain", "upload",
                                               "restore", ("step 0", 2000))),
}


@pytest.mark.parametrize("name", sorted(HAND_SCRIPTS))
def test_live_bound_covers_the_particles_alive_hand_scripts(ledger, name):
    g, (lines, at_build) = HAND_SCRIPTS[name]
    assert bound_shortfalls(ledger(g, lines), lines, at_build) == []


def test_live_bound_covers_the_particles_alive_random_scripts(ledger):
    """240 scripts with a world beside them: worlds 1 and 2, explosions on and off, run-ahead 0 and 1.  The generator must
    put fill, upload and restore behind an unread record often enough for the property to mean something."""
    met, behind = set(), {"fill": 0, "upload": 0, "restore": 0}
    for k in range(240):
        rng = random.Random(12000 + k)
        g = random_config(rng, k)
        met.add((g.world, g.expl, g.ra))
        world = World(rng, g)
        lines = random_script(rng, g, world=world)
        states = ledger(g, lines)
        assert bound_shortfalls(states, lines, world.at_build) == [], (k, cfg_line(g), lines)
        for line, before in zip(lines[1:], states):
            op = line.split()[0]
            if op in behind and int(before["seq"]) > int(before["seen"]):
                behind[op] += 1
    assert len(met) == 8
    assert min(behind.values()) >= 20, behind


# ---- named cases ----
def test_run_ahead_reads_the_step_before_and_this_one_if_it_has_arrived(ledger):
    g = config(ra=1)
    s = ledger(g, ["step 0", rec_line(record(1, live=10)), "step 0", rec_line(record(2, live=20)), rec_line(record(3, live=30)), "step 0"])
    assert [(v["seq"], v["seen"]) for v in s] == [("1", "0"), ("1", "0"), ("2", "1"), ("2", "1"), ("2", "1"), ("3", "3")]
    assert s[2]["live"] == "10" and s[5]["live"] == "30"
    # ... and without run-ahead every step's own record
    s = ledger(config(ra=0), [rec_line(record(1, live=10)), "step 0", rec_line(record(2, live=20)), "step 0"])
    assert [(v["seq"], v["seen"]) for v in s] == [("0", "0"), ("1", "1"), ("1", "1"), ("2", "2")]


def test_two_pass_step_rescales_tasks_and_packs_for_its_own_record_only(ledger):
    g = config(world=2, ra=0, comp=900, comp_int=300, comp_rest=600, cap0=16, xfer=16, capmax=16)
    r = dict(n_tasks2=1000, n_merged=200)
    s = ledger(g, [rec_line(record(1, **r)), "step 1", rec_line(record(2, **r)), "step 0"])
    # step 1 ran in two passes: (1000 + 200) * 900 / 600 tasks, 200 * 900 / 600 packs (in steps of 64: 320)
    assert s[1]["hint"] == "1800/320"
    assert s[3]["hint"] == "1200/256"


def test_inject_counts_until_the_record_of_the_next_step_is_read(ledger):
    g = config(ra=1, slots=100000)
    s = ledger(g, ["step 0", "inject 500", rec_line(record(1, live=1000)), "step 0", rec_line(record(2, live=1100)), "step 0"])
    bound = [v["bound"].split("/")[1] for v in s]
    assert bound[1] == "500"                        # (nothing read yet: the bound of the empty context + the inject)
    assert bound[3] == "1500"                       # record 1 (its step was enqueued before the inject) does not count it: 1000 + 500
    assert bound[5] == "1100"                       # record 2 is the first that does: the tally is dropped as it is read


def test_capacity_decision_is_adopted_two_steps_on_and_clamped(ledger):
    for ra in (0, 1):
        g = config(world=2, ra=ra, xfer=16, cap0=16, capmax=1024)
        lines = ["build", "step 0", rec_line(record(1, xfer_cap_next=300)), "build", "step 0", rec_line(record(2, xfer_cap_next=5000)),
                 "build", "step 0", rec_line(record(3, xfer_cap_next=4)), "build", "step 0", rec_line(record(4)), "build", "step 0"]
        if ra == 0:                                 # (every step waits for its own record: it must be there)
            lines = ["build", rec_line(record(1, xfer_cap_next=300)), "step 0", "build", rec_line(record(2, xfer_cap_next=5000)), "step 0",
                     "build", rec_line(record(3, xfer_cap_next=4)), "step 0", "build", rec_line(record(4)), "step 0", "build", "step 0"]
            lines.insert(-1, rec_line(record(5)))
        s = ledger(g, lines)
        caps = [v["cap"] for v, line in zip(s, lines) if line == "build"]
        assert caps == ["16", "16", "300", "1024", "16"], ra      # builds of steps 1 .. 5: step 1's decision at step 3, step 2's clamped, step 3's clamped


def test_verdict_met_by_a_quiet_drain_is_returned_by_the_next_reporting_call_once(ledger):
    s = ledger(config(ra=1), ["step 0", rec_line(record(1, error=64)), "drainq", "drainq", "drain", "drain"])
    assert [(v["pending"], v["ret"]) for v in s[2:]] == [("64", "0"), ("64", "0"), ("0", "64"), ("0", "0")]
    assert s[4]["err"] == "step-1"
    # a slab: only what was in the all-gathered status records
    s = ledger(config(world=2, ra=1, cap0=16, xfer=16, capmax=16), ["step 0", rec_line(record(1, error=64)), "drain",
                                                                 "step 0", rec_line(record(2, error=64, status_error=64)), "drain"])
    assert [v["ret"] for v in s] == ["0", "0", "0", "0", "0", "64"]


def test_upload_makes_the_bound_unknown_until_the_next_record(ledger):
    g = config(ra=0, slots=5000)
    s = ledger(g, ["fill 100", "upload", "fill 50", rec_line(record(1, live=150, n_moves=7)), "step 0"])
    assert [v["bound"] for v in s] == ["65536/100", "65536/5000", "65536/5000", "65536/5000", "65536/157"]
    assert s[1]["hint"] == "%d/0" % (5000 // 64 + 512)


def test_snapshot_restore_brings_back_the_saved_bound(ledger):
    s = ledger(config(ra=0), ["fill 100", "save", "fill 23", "upload", "restore"])
    assert [v["bound"].split("/")[1] for v in s] == ["100", "100", "123", "100000", "100"]


def test_today_an_error_record_that_arrived_early_is_released_by_the_call_that_enqueued_its_step(ledger):
    """ADVICE.md, first finding, as the code stands: with run-ahead 1 the call that enqueues step s waits for record s - 1 only,
    but reads record s too if it is there, and returns its verdict; a rank whose record s comes later returns it one call on."""
    g = config(world=2, ra=1, cap0=16, xfer=16, capmax=16)
    bad = rec_line(record(2, status_error=64))
    early = ledger(g, ["step 0", rec_line(record(1)), bad, "step 0", rec_line(record(3)), "step 0"])
    late = ledger(g, ["step 0", rec_line(record(1)), "step 0", bad, rec_line(record(3)), "step 0"])
    assert [v["ret"] for v in early] == ["0", "0", "0", "64", "0", "0"]      # from the call that enqueued step 2
    assert [v["ret"] for v in late] == ["0", "0", "0", "0", "0", "64"]       # from the call that enqueued step 3


def test_a_script_that_waits_for_a_record_that_is_not_there_is_refused(ledger):
    out = subprocess.run([ledger.exe], input=cfg_line(config(ra=0)) + "\nstep 0\n", capture_output=True, text=True)
    assert out.returncode == 2 and out.stdout.splitlines()[-1] == "STALL 1" and out.stderr == ""
