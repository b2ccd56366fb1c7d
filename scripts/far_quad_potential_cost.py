"""What the quadrupole form of psamd_potential and psamd_probe costs (PSAMD_POTENTIAL_FAR | PSAMD_POTENTIAL_QUADRUPOLE,
PSAMD_PROBE_FAR | PSAMD_PROBE_QUADRUPOLE on a PSAMD_FLAG_FAR_QUADRUPOLE context) beside the far form on a pyramid context
(PSAMD_POTENTIAL_FAR, PSAMD_PROBE_FAR), in the same run.  The protocol is scripts/far_potential_cost.py's.

    python scripts/far_quad_potential_cost.py [--reps K] [--out profiles/far_quad_potential_cost.txt]

One MI355X, a uniform cloud of N = 2^20 on 16^3 cells, default constants; both contexts filled with the same cloud.  One frame is
built (init_iframe, build_grid) and K times each of
    psamd_potential into a device array of phi
    psamd_probe, ACC | PHI, 65 536 probes on the first 65 536 particles' own positions
    psamd_probe, ACC | PHI, 65 536 probes on a regular grid of 32 x 32 x 64 points
is timed with a host clock around the call + psamd_synchronize (the stream idle before it; two calls first to warm up).  The calls
form the moments themselves -- ten planes a level on the quadrupole context, four on the pyramid --; that is in their time."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime)

import particlesystem_amd as ps  # noqa: E402

MODELS = (("quadrupoles", "far_quadrupole", ps.FLAG_FAR_PYRAMID | ps.FLAG_FAR_QUADRUPOLE, ps.POTENTIAL_FAR | ps.POTENTIAL_QUADRUPOLE,
           ps.PROBE_FAR | ps.PROBE_QUADRUPOLE),
          ("pyramid", "far_pyramid", ps.FLAG_FAR_PYRAMID, ps.POTENTIAL_FAR, ps.PROBE_FAR))
CALLS = ("potential", "probe_on_particles", "probe_on_grid")
PROBES = 65536


def clock(g, call, reps):
    for _ in range(2):
        call()
    g.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        g.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def measure(n, reps):
    dev = torch.device("cuda", 0)
    res = {"n": n, "reps": reps, "probes": PROBES}
    xyz = age = None
    rng = np.random.default_rng(18)
    for _, key, flags, pot_bits, probe_bits in MODELS:
        g = ps.ParticleSystem(ps.default_config(device=0, flags=flags))
        if xyz is None:
            xyz = g.uniform_cloud(n, 12345)
            age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
            half = g.sizes.grid_dim * 2.5
            k = (np.stack(np.meshgrid(np.arange(32), np.arange(32), np.arange(64), indexing="ij"), -1).reshape(-1, 3) + 0.5)
            grid = (k / np.array([32, 32, 64]) * 2 * half - half).astype(np.float32)
        g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
        g.init_iframe(); g.build_grid()
        phi = torch.zeros(g.owned_slots(), dtype=torch.float32, device=dev)
        rec = torch.zeros(64, dtype=torch.uint8, device=dev)
        spec = ps.Potential(flags=pot_bits, phi=phi.data_ptr(), capacity=phi.numel(), result_dev=rec.data_ptr())
        out4 = torch.zeros((PROBES, 4), dtype=torch.float32, device=dev)

        def pos4(p):
            q = np.zeros((PROBES, 4), np.float32)
            q[:, :3] = p
            return torch.from_numpy(q).to(dev)
        own, reg = pos4(xyz[:PROBES]), pos4(grid)
        fields = ps.PROBE_ACC | ps.PROBE_PHI | probe_bits
        specs = [ps.ProbeSpec(fields=fields, pos4=p.data_ptr(), max_count=PROBES, out4=out4.data_ptr()) for p in (own, reg)]
        torch.cuda.synchronize()
        ck = lambda st: g._ck(st)
        v = {"potential": clock(g, lambda: ck(g.lib.psamd_potential(g.h, C.byref(spec))), reps),
             "probe_on_particles": clock(g, lambda: ck(g.lib.psamd_probe(g.h, C.byref(specs[0]))), reps),
             "probe_on_grid": clock(g, lambda: ck(g.lib.psamd_probe(g.h, C.byref(specs[1]))), reps)}
        v["listed"] = g.potential_result()["listed"]
        v["served"] = g.probe_result()["served"]
        g.calc_forces()
        res[key] = v
        print(key, json.dumps(v), flush=True)
        g.close()
    res["ratio"] = {k: res["far_quadrupole"][k]["ms"] / res["far_pyramid"][k]["ms"] for k in CALLS}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "far_quad_potential_cost.txt"))
    a = ap.parse_args()
    res = measure(1 << 20, a.reps)
    with open(a.out, "w") as fo:
        fo.write("The quadrupole form of psamd_potential and psamd_probe (PSAMD_POTENTIAL_FAR | PSAMD_POTENTIAL_QUADRUPOLE, PSAMD_PROBE_FAR |\n"
                 "PSAMD_PROBE_QUADRUPOLE on a quadrupole context) beside the far form on a pyramid context, in the same run: one MI355X,\n"
                 "uniform cloud of N = %d on 16^3 cells, default constants.  Host clock around the call + psamd_synchronize, median of %d\n"
                 "(min .. max), ms; %d probes, ACC | PHI.  python scripts/far_quad_potential_cost.py\n\n"
                 % (res["n"], res["reps"], PROBES))
        fo.write("%-18s %-26s %-26s %-26s\n" % ("", "potential", "probes on particles", "probes on a grid"))
        for name, key, _, _, _ in MODELS:
            v = res[key]
            fo.write("%-18s " % name + " ".join("%8.3f (%6.3f .. %6.3f)" % (v[k]["ms"], v[k]["min"], v[k]["max"]) for k in CALLS) + "\n")
        fo.write("%-18s " % "ratio" + " ".join("%8.2f %-17s" % (res["ratio"][k], "") for k in CALLS) + "\n\n")
        fo.write(json.dumps(res, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
