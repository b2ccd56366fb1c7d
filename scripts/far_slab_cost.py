"""What the far field costs on slabs (PSAMD_FLAG_FAR_SLAB), as far as ONE MI355X can show it.

    python scripts/far_slab_cost.py [--steps K] [--baseline-lib PATH] [--out profiles/far_slab_cost.txt]
    python scripts/far_slab_cost.py --part one|slabs --model pyramid|quadrupole [--slab-flag] [--steps K]      (one measurement, one JSON line)

N = 2^20 on 16^3 cells, uniform cloud, default constants, for the pyramid and for quadrupoles on it:

  one context   ms per step by scripts/far_monopole_cost.py's protocol (every step from the same fill, host clock around
                psamd_step(1) + psamd_synchronize, then as many steps with the pair stage's own timer): without the flag, with
                PSAMD_FLAG_FAR_SLAB at world 1 -- the same kernels, so the two must agree within the spread -- and, with
                --baseline-lib, the same from another build of the library (the commit before the flag existed; PSAMD_LIB).
                Every measurement is a process of its own, the variants alternate, two rounds: the spread between rounds of
                one variant is what a difference between variants is held against.
  eight slabs   all eight ranks of a world of 8 in one process on the one GPU (step_local: the messages are copied rank to
                rank through the host; one_at_a_time: a rank's pair stage has the GPU to itself, as on a GPU of its own),
                every step from the same fill, each rank's own pair-stage timer, beside one eighth of the one context's.  A PROJECTION: eight GPUs would run the ranks side by side and move the messages over the
                fabric, which this does not measure.

The added launches (the own cells' sums in slab_build; the scatter with level 0 and the upper levels in slab_pairs) are timed by
a kernel trace, in runs of their own (no counters): for MODEL in pyramid, quadrupole and PART in one, slabs

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/MODEL_PART -o t -- python scripts/far_slab_cost.py --part PART --model MODEL --steps 10
    python scripts/far_slab_cost.py --kernel-trace DIR      (the table: per kernel of the pair stage and per rank, median us)

A context has a stream of its own, so the trace's stream ids, in the order of creation, are the ranks."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

N = 1 << 20
WORLD = 8


def flags_of(ps, model, slab_flag):
    f = ps.FLAG_FAR_PYRAMID | (ps.FLAG_FAR_QUADRUPOLE if model == "quadrupole" else 0)
    return f | (ps.FLAG_FAR_SLAB if slab_flag else 0)


def the_cloud(g, np):
    rng = np.random.default_rng(18)
    return g.uniform_cloud(N, 12345), rng.uniform(15 / 7, 7.5, N).astype(np.float32)


def part_one(a):
    import numpy as np
    import torch  # noqa: F401  (before the library: one HIP runtime)
    import particlesystem_amd as ps
    from far_monopole_cost import timed
    g = ps.ParticleSystem(ps.default_config(device=0, flags=flags_of(ps, a.model, a.slab_flag)))
    xyz, age = the_cloud(g, np)
    g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    res = timed(g, a.steps, 3)
    g.close()
    return res


def part_slabs(a):
    import numpy as np
    import torch  # noqa: F401
    import particlesystem_amd as ps
    from particlesystem_amd.slab import step_local
    # (the long-range force moves the whole uniform cloud inwards by up to a cell a step: a quarter of a rank's particles change
    # owner in the first steps from the fill, more than the transfer messages' default room, which follows the traffic two
    # steps behind and starts anew with every restore)
    ranks = [ps.ParticleSystem(ps.default_config(device=0, flags=flags_of(ps, a.model, True), rank=r, world=WORLD, xfer_cap=1 << 17))
             for r in range(WORLD)]
    xyz, age = the_cloud(ranks[0], np)
    for g in ranks:
        g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
        g.snapshot_save()
    for _ in range(2):                 # warm-up, each step from the fill too: a run of steps crowds the cells past their lists
        for g in ranks:
            g.snapshot_restore()
        step_local(ranks, one_at_a_time=True)
    for g in ranks:
        g.synchronize()
        g.set_timing(True)
    for _ in range(a.steps):
        for g in ranks:
            g.snapshot_restore()
        step_local(ranks, one_at_a_time=True)
        for g in ranks:
            g.synchronize()
    pairs = []
    for g in ranks:
        t, launches = g.timing()
        pairs.append(t["pairs"] / max(launches, 1) / 1e3)
    res = {"pairs_timer_ms_per_rank": pairs, "steps": a.steps, "allg_bytes": ranks[0].msg_bytes(ps.MSG_ALLG_OUT)}
    for g in ranks:
        g.close()
    return res


# the kernels psamd_slab_pairs launches (one context: the pair stage's), and k_cell_moments (a slab: the OWN form, in slab_build)
STAGE = ("k_cell_moments", "k_halo_prefix_in", "k_halo_bodies_in", "k_far_scatter", "k_level_moments", "k_chunk_census", "k_collide_cell",
         "k_plan_force", "k_pack_windows", "k_pairs_balanced", "k_allp_prefix", "k_allp_dense", "k_far_walk", "k_allpairs_combine", "k_pack_force")


def trace_table(path, steps):
    """{kernel: [median us per step and stream, streams in the order of creation]} over the last `steps` steps of every stream
    that ran a far walk; a kernel launched more than once a step (the levels) counts as the sum of its launches"""
    import csv
    import glob
    import re
    import statistics
    per = {}
    for f in glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = re.match(r"(?:void )?(?:psamd::)?(\w+)", r["Kernel_Name"]).group(1)
            if name in STAGE:
                per.setdefault(int(r["Stream_Id"]), {}).setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    streams = sorted(s for s in per if "k_far_walk" in per[s])
    out = {}
    for name in STAGE:
        row = []
        for s in streams:
            d = sorted(per[s].get(name, []))
            k = len(d) // len(per[s]["k_far_walk"])                      # launches a step
            d = d[len(d) - k * steps:]
            row.append(statistics.median(sum(e - b for b, e in d[i * k:(i + 1) * k]) / 1e3 for i in range(steps)) if k else 0.0)
        if any(row):
            out[name] = row
    return out


def print_traces(path, steps):
    for model in ("pyramid", "quadrupole"):
        one, slabs = (trace_table(os.path.join(path, "%s_%s" % (model, part)), steps) for part in ("one", "slabs"))
        print("%s: kernels of the pair stage, median us a step over %d steps; k_cell_moments on slabs is the OWN form in slab_build" % (model, steps))
        print("  %-20s %9s %9s   %s" % ("", "one ctx", "ranks' sum", "rank 0 .. 7"))
        tot_one, tot = 0.0, [0.0] * len(next(iter(slabs.values())))
        for name in STAGE:
            if name not in one and name not in slabs:
                continue
            a, row = one.get(name, [0.0])[0], slabs.get(name, [0.0] * len(tot))
            print("  %-20s %9.1f %9.1f   %s" % (name, a, sum(row), " ".join("%6.1f" % v for v in row)))
            if name != "k_cell_moments":
                tot_one, tot = tot_one + a, [t + v for t, v in zip(tot, row)]
            else:
                tot_one += a
        print("  %-20s %9.1f %9.1f   %s\n" % ("the stage's kernels", tot_one, sum(tot), " ".join("%6.1f" % v for v in tot)))


def child(args, lib=None):
    env = dict(os.environ)
    if lib:
        env["PSAMD_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, stdout=subprocess.PIPE, text=True, timeout=600, check=True)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--part", choices=("one", "slabs"))
    ap.add_argument("--model", choices=("pyramid", "quadrupole"), default="pyramid")
    ap.add_argument("--slab-flag", action="store_true")
    ap.add_argument("--baseline-lib", default="", help="libpsamd.so of the commit before PSAMD_FLAG_FAR_SLAB")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "far_slab_cost.txt"))
    ap.add_argument("--kernel-trace", default="", help="a directory of kernel traces of --part runs (see above): print their table")
    a = ap.parse_args()
    if a.kernel_trace:
        print_traces(a.kernel_trace, a.steps if a.steps != 20 else 10)
        return
    if a.part:
        print(json.dumps(part_one(a) if a.part == "one" else part_slabs(a)))
        return
    res = {}
    for model in ("pyramid", "quadrupole"):
        base = ["--model", model, "--steps", str(a.steps)]
        variants = [("no flag", base + ["--part", "one"], None), ("FAR_SLAB, world 1", base + ["--part", "one", "--slab-flag"], None)]
        if a.baseline_lib:
            variants.insert(0, ("baseline build", base + ["--part", "one"], a.baseline_lib))
        one = {name: [] for name, _, _ in variants}
        for _ in range(2):
            for name, args, lib in variants:
                one[name].append(child(args, lib))
                print(model, name, json.dumps(one[name][-1]), flush=True)
        res[model] = {"one_context": one, "slabs": child(base + ["--part", "slabs"])}
        print(model, "slabs", json.dumps(res[model]["slabs"]), flush=True)
    with open(a.out, "w") as fo:
        fo.write("The far field on slabs (PSAMD_FLAG_FAR_SLAB), one MI355X, N = 2^20 on 16^3 cells, uniform cloud, default constants.\n"
                 "python scripts/far_slab_cost.py%s; every figure a process of its own, %d steps each from the same fill.\n"
                 "The eight-slab figures are PROJECTIONS from eight ranks stepped on one GPU.\n\n" % (" --baseline-lib ..." if a.baseline_lib else "", a.steps))
        for model, r in res.items():
            fo.write("%s, one context: ms per step, median (min .. max), pair-stage timer; two rounds, variants alternating\n" % model)
            for name, runs in r["one_context"].items():
                for k, v in enumerate(runs):
                    fo.write("  %-20s round %d  %8.3f  (%.3f .. %.3f)  pairs timer %8.3f\n" % (name, k + 1, v["ms_per_step"], v["min"], v["max"], v["pairs_timer_ms"]))
            eighth = r["one_context"]["no flag"][0]["pairs_timer_ms"] / WORLD
            s = r["slabs"]
            fo.write("%s, eight slabs on one GPU, one rank at a time: pair-stage timer per rank, ms: %s\n" % (model, " ".join("%.3f" % v for v in s["pairs_timer_ms_per_rank"])))
            fo.write("  one eighth of the one context's pair timer: %.3f ms; the block of cell sums a rank sends: %d bytes\n\n" % (eighth, s["allg_bytes"]))
        fo.write(json.dumps(res, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
