"""What a step costs with far monopoles beside the cutoff step and the all-pairs step, and how far its force is from
true long-range gravity.

    python scripts/far_monopole_cost.py [--steps K] [--out profiles/far_monopole_cost.txt]

One MI355X, N = 2^20 uniform cloud, default constants (16^3 cells, 256 to a cell).  Three contexts filled with the same
cloud: PSAMD_FLAG_FAR_MONOPOLE, no flag (the cutoff step: the code path of a context without the flag is unchanged), and
PSAMD_FLAG_ALL_PAIRS.  Each is warmed up (3 steps; all-pairs 1), then K times (all-pairs: K / 4) put back to the fill
(snapshot_restore) and stepped once, a host clock around psamd_step(1) + psamd_synchronize: the step at the full N, median
with the spread beside it.  Then, timing on, as many such steps again for the pair stage's own timer (force pass + far pass).
Deviation: one frame of the far-monopole context at the fill, 200 served particles sampled as
tests/test_gpu_extras.py::test_all_pairs_at_config1_size samples them, |a - a_direct| / |a_direct| against an fp64 direct sum
over all 2^20 bodies; the same for the cutoff context's records."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: F401, E402  (before the library: one HIP runtime)

import far_model as F  # noqa: E402
import particlesystem_amd as ps  # noqa: E402

N = 1 << 20


def timed(g, steps, warm):
    """ms of ONE step from the fill, `steps` times over (a run of steps would thin the cloud out: at the default collision
    radius two fifths of it collide in the first step); then the pair stage's own timer over as many such steps"""
    g.snapshot_save()
    g.step(warm)
    g.synchronize()
    ms = []
    for timing in (False, True):
        g.set_timing(timing)
        for _ in range(steps):
            g.snapshot_restore()
            g.synchronize()
            t0 = time.perf_counter()
            g.step(1)
            g.synchronize()
            if not timing:
                ms.append((time.perf_counter() - t0) * 1e3)
    t, launches = g.timing()
    g.set_timing(False)
    g.snapshot_restore()
    return {"ms_per_step": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "steps": steps,
            "pairs_timer_ms": t["pairs"] / max(launches, 1) / 1e3, "collide_timer_ms": t["collide"] / max(launches, 1) / 1e3}


def records(g):
    g.init_iframe(); g.build_grid(); g.calc_forces_pairs()
    rows = g.download_cellgrid()
    order = np.concatenate([row[1:1 + row[0]] for row in rows])
    f = g.download_force4(0, len(order))
    g.calc_forces_apply()
    return order, f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "far_monopole_cost.txt"))
    a = ap.parse_args()
    res = {"n": N, "steps": a.steps}
    xyz = age = ids = None
    dev = {}
    rng = np.random.default_rng(18)
    for name, flags, steps, warm in (("far_monopole", ps.FLAG_FAR_MONOPOLE, a.steps, 3), ("cutoff", 0, a.steps, 3),
                                     ("all_pairs", ps.FLAG_ALL_PAIRS, max(1, a.steps // 4), 1)):
        g = ps.ParticleSystem(ps.default_config(device=0, flags=flags))
        if xyz is None:
            xyz = g.uniform_cloud(N, 12345)
            age = rng.uniform(15 / 7, 7.5, N).astype(np.float32)
        ids = g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
        res[name] = timed(g, steps, warm)
        print(name, json.dumps(res[name]), flush=True)
        if name != "all_pairs":
            dev[name] = records(g)
        g.close()
    where = np.empty(int(ids.max()) + 1, np.int64)
    where[ids] = np.arange(N)
    order, f = dev["far_monopole"]
    served = np.nonzero(f[:, 3].view(np.int32) == 0)[0]
    pick = rng.choice(served, 200, replace=False)
    idx = where[order[pick]]
    want = F.direct(xyz, np.full(N, 60.0, np.float32), 0.2, idx, chunk=8)
    for name in ("far_monopole", "cutoff"):
        o, ff = dev[name]
        assert np.array_equal(o, order)
        rel = F.rel_dev(ff[pick, :3].astype(np.float64), want)
        res[name]["deviation_from_direct_sum"] = {"median": float(np.median(rel)), "max": float(rel.max()), "sampled": 200}
    far, cut, allp = (res[k]["ms_per_step"] for k in ("far_monopole", "cutoff", "all_pairs"))
    res["far_over_cutoff"] = far / cut
    res["all_pairs_over_far"] = allp / far
    with open(a.out, "w") as fo:
        fo.write("A step with far monopoles (PSAMD_FLAG_FAR_MONOPOLE) beside the cutoff step and the all-pairs step, one MI355X,\n"
                 "N = 2^20 uniform cloud, default constants (16^3 cells).  Host clock around psamd_step(1) + psamd_synchronize, every\n"
                 "step from the same fill (snapshot_restore): median of %d steps (min .. max; all-pairs %d steps).  ms per step.\n"
                 "pairs timer: the pair stage's own timer (force pass + far pass) over the same steps.\n\n" % (a.steps, max(1, a.steps // 4)))
        for name, key in (("far monopoles", "far_monopole"), ("cutoff (no flag)", "cutoff"), ("all-pairs", "all_pairs")):
            v = res[key]
            fo.write("%-20s %9.3f   (%.3f .. %.3f)   pairs timer %9.3f\n" % (name, v["ms_per_step"], v["min"], v["max"], v["pairs_timer_ms"]))
        fo.write("\nfar monopoles / cutoff   %.2f\nall-pairs / far monopoles %.1f\n" % (res["far_over_cutoff"], res["all_pairs_over_far"]))
        fo.write("\nDeviation of |a| from an fp64 direct sum over all 2^20 bodies, 200 served particles of the first frame:\n")
        for name, key in (("far monopoles", "far_monopole"), ("cutoff (no flag)", "cutoff")):
            d = res[key]["deviation_from_direct_sum"]
            fo.write("%-20s median %.3g   max %.3g\n" % (name, d["median"], d["max"]))
        fo.write("\n" + json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
