"""What quadrupoles on the pyramid cost a step, and what they buy: PSAMD_FLAG_FAR_PYRAMID | PSAMD_FLAG_FAR_QUADRUPOLE beside the
pyramid of monopoles and the cutoff step of the same build.

    python scripts/far_quadrupole_cost.py [--steps K] [--small] [--out profiles/far_quadrupole_cost.txt]

The protocol is scripts/far_pyramid_cost.py's (far_monopole_cost.py's timed() and records() are used as they are): one MI355X,
a uniform cloud, default constants; three contexts filled with the same cloud -- the cutoff step (no flag), the pyramid, the
pyramid with quadrupoles -- each warmed up with 3 steps, then K times put back to the fill and stepped once with a host clock
around psamd_step(1) + psamd_synchronize; then as many such steps again with timing on for the pair stage's own timer.  The
quadrupole step is set against the pyramid step of the same run.  Deviation: one frame at the fill, 200 served particles,
|a - a_direct| / |a_direct| against an fp64 direct sum over all bodies.  N = 2^20 on 16^3 cells and N = 2^22 on 24^3 cells
(chunk_factor 6); --small leaves the second size out."""
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

MODELS = (("cutoff (no flag)", "cutoff", 0), ("pyramid", "far_pyramid", ps.FLAG_FAR_PYRAMID),
          ("pyramid + quadrupoles", "far_quadrupole", ps.FLAG_FAR_PYRAMID | ps.FLAG_FAR_QUADRUPOLE))


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
    q, p, c = res["far_quadrupole"], res["far_pyramid"], res["cutoff"]
    res["quadrupole_over_pyramid"] = q["ms_per_step"] / p["ms_per_step"]
    res["quadrupole_over_cutoff"] = q["ms_per_step"] / c["ms_per_step"]
    res["pairs_timer_quadrupole_over_pyramid"] = q["pairs_timer_ms"] / p["pairs_timer_ms"]
    res["median_deviation_quadrupole_over_pyramid"] = q["deviation_from_direct_sum"]["median"] / p["deviation_from_direct_sum"]["median"]
    return res


def report(fo, res):
    fo.write("N = %d, levels %s: ms per step, median of %d steps (min .. max); pairs timer: the pair stage's own timer\n"
             % (res["n"], res["levels"], res["steps"]))
    for name, key, _ in MODELS:
        v = res[key]
        fo.write("%-24s %9.3f   (%.3f .. %.3f)   pairs timer %9.3f\n" % (name, v["ms_per_step"], v["min"], v["max"], v["pairs_timer_ms"]))
    fo.write("quadrupoles / pyramid    %.3f of the step, %.3f of the pairs timer\nquadrupoles / cutoff     %.2f\n"
             % (res["quadrupole_over_pyramid"], res["pairs_timer_quadrupole_over_pyramid"], res["quadrupole_over_cutoff"]))
    fo.write("deviation of |a| from an fp64 direct sum over all %d bodies, 200 served particles of the first frame:\n" % res["n"])
    for name, key, _ in MODELS:
        d = res[key]["deviation_from_direct_sum"]
        fo.write("%-24s median %.3g   max %.3g\n" % (name, d["median"], d["max"]))
    fo.write("median, quadrupoles / pyramid  %.2f\n\n" % res["median_deviation_quadrupole_over_pyramid"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="N = 2^20 on 16^3 cells only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "far_quadrupole_cost.txt"))
    a = ap.parse_args()
    runs = [measure(1 << 20, {}, a.steps)]
    if not a.small:
        runs.append(measure(1 << 22, dict(max_particles_num=1 << 22, chunk_factor=6, chunk_dim=4), a.steps))
    with open(a.out, "w") as fo:
        fo.write("A step with quadrupoles on the pyramid (PSAMD_FLAG_FAR_PYRAMID | PSAMD_FLAG_FAR_QUADRUPOLE) beside the pyramid of monopoles\n"
                 "and the cutoff step of the same build, one MI355X, uniform cloud, default constants.  Host clock around psamd_step(1) +\n"
                 "psamd_synchronize, every step from the same fill (snapshot_restore).  python scripts/far_quadrupole_cost.py%s\n\n"
                 % (" --small" if a.small else ""))
        for res in runs:
            report(fo, res)
        fo.write(json.dumps(runs, indent=1) + "\n")
    print(json.dumps(runs))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
