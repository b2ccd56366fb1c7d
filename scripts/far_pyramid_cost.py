"""What a step costs with the pyramid of monopoles beside the far-monopole step and the cutoff step of the same build, and how
far its force is from true long-range gravity.

    python scripts/far_pyramid_cost.py [--steps K] [--big] [--out profiles/far_pyramid_cost.txt]

The protocol is scripts/far_monopole_cost.py's (its timed() and records() are used as they are): one MI355X, a uniform cloud,
default constants; three contexts filled with the same cloud -- PSAMD_FLAG_FAR_PYRAMID, PSAMD_FLAG_FAR_MONOPOLE and no flag
(the cutoff step) -- each warmed up with 3 steps, then K times put back to the fill and stepped once with a host clock around
psamd_step(1) + psamd_synchronize; then as many such steps again with timing on for the pair stage's own timer.  Deviation:
one frame at the fill, 200 served particles, |a - a_direct| / |a_direct| against an fp64 direct sum over all bodies.
N = 2^20 on 16^3 cells; with --big also N = 2^22 on 24^3 cells (chunk_factor 6), where the flat method has 40 times the
pyramid's far bodies."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: F401, E402  (before the library: one HIP runtime)

import far_model as F  # noqa: E402
import particlesystem_amd as ps  # noqa: E402
from far_monopole_cost import records, timed  # noqa: E402

MODELS = (("pyramid", "far_pyramid", ps.FLAG_FAR_PYRAMID), ("far monopoles", "far_monopole", ps.FLAG_FAR_MONOPOLE),
          ("cutoff (no flag)", "cutoff", 0))


def measure(n, over, steps, sampled=200):
    res = {"n": n, "steps": steps, "levels": ps.far_levels(ps.default_config(**over))}
    xyz = age = ids = None
    dev = {}
    rng = np.random.default_rng(18)
    for _, key, flags in MODELS:
        g = ps.ParticleSystem(ps.default_config(device=0, flags=flags, **over))
        if xyz is None:
            xyz = g.uniform_cloud(n, 12345)
            age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
        ids = g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
        res[key] = timed(g, steps, 3)
        print(n, key, json.dumps(res[key]), flush=True)
        dev[key] = records(g)
        g.close()
    where = np.empty(int(ids.max()) + 1, np.int64)
    where[ids] = np.arange(n)
    order, f = dev["far_pyramid"]
    served = np.nonzero(f[:, 3].view(np.int32) == 0)[0]
    pick = rng.choice(served, sampled, replace=False)
    want = F.direct(xyz, np.full(n, 60.0, np.float32), 0.2, where[order[pick]], chunk=8 if n <= 1 << 20 else 2)
    for _, key, _ in MODELS:
        o, ff = dev[key]
        assert np.array_equal(o, order)
        rel = F.rel_dev(ff[pick, :3].astype(np.float64), want)
        res[key]["deviation_from_direct_sum"] = {"median": float(np.median(rel)), "max": float(rel.max()), "sampled": sampled}
    res["pyramid_over_far_monopole"] = res["far_pyramid"]["ms_per_step"] / res["far_monopole"]["ms_per_step"]
    res["pyramid_over_cutoff"] = res["far_pyramid"]["ms_per_step"] / res["cutoff"]["ms_per_step"]
    return res


def report(fo, res):
    fo.write("N = %d, levels %s: ms per step, median of %d steps (min .. max); pairs timer: the pair stage's own timer\n"
             % (res["n"], res["levels"], res["steps"]))
    for name, key, _ in MODELS:
        v = res[key]
        fo.write("%-20s %9.3f   (%.3f .. %.3f)   pairs timer %9.3f\n" % (name, v["ms_per_step"], v["min"], v["max"], v["pairs_timer_ms"]))
    fo.write("pyramid / far monopoles  %.2f\npyramid / cutoff         %.2f\n" % (res["pyramid_over_far_monopole"], res["pyramid_over_cutoff"]))
    fo.write("deviation of |a| from an fp64 direct sum over all %d bodies, 200 served particles of the first frame:\n" % res["n"])
    for name, key, _ in MODELS:
        d = res[key]["deviation_from_direct_sum"]
        fo.write("%-20s median %.3g   max %.3g\n" % (name, d["median"], d["max"]))
    fo.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--big", action="store_true", help="also N = 2^22 on 24^3 cells")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "far_pyramid_cost.txt"))
    a = ap.parse_args()
    runs = [measure(1 << 20, {}, a.steps)]
    if a.big:
        runs.append(measure(1 << 22, dict(max_particles_num=1 << 22, chunk_factor=6, chunk_dim=4), a.steps))
    with open(a.out, "w") as fo:
        fo.write("A step with the pyramid of monopoles (PSAMD_FLAG_FAR_PYRAMID) beside the far-monopole step and the cutoff step of the\n"
                 "same build, one MI355X, uniform cloud, default constants.  Host clock around psamd_step(1) + psamd_synchronize, every\n"
                 "step from the same fill (snapshot_restore).  python scripts/far_pyramid_cost.py%s\n\n" % (" --big" if a.big else ""))
        for res in runs:
            report(fo, res)
        fo.write(json.dumps(runs, indent=1) + "\n")
    print(json.dumps(runs))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
