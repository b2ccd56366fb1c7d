"""What psamd_deposit costs on the default N = 2^20 uniform cloud, 16^3 cells (one MI355X).

    python scripts/deposit_cost.py [--reps R] [--warmup W] [--out profiles/deposit_cost.txt]

The protocol of the far-potential figures: one built frame (a cloud filled and stepped twice, init_iframe, build_grid), on it
psamd_deposit at refine 1, 2 and 4 and, beside them in the same run, psamd_potential (the result alone).  Every figure is a
host clock around the call plus psamd_synchronize, with an idle stream before it, after warm-up calls.  Before the timing each
refine's array is checked to come out the same bytes twice and to hold the mass its record reports."""
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


def timed(g, call, reps, warmup):
    """microseconds of call() + synchronize from an idle stream: (median, min, max)"""
    us = []
    for rep in range(warmup + reps):
        g.synchronize()
        t0 = time.perf_counter()
        call()
        g.synchronize()
        if rep >= warmup:
            us.append((time.perf_counter() - t0) * 1e6)
    return {"us_median": float(np.median(us)), "us_min": float(np.min(us)), "us_max": float(np.max(us))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deposit_cost.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = 1 << 20
    g = ps.ParticleSystem(ps.default_config(device=0))
    G = int(g.sizes.grid_dim)
    g.fill_particles(g.uniform_cloud(n, 12345), age=np.float32(2.0), fert_age=np.float32(1e6))
    g.step(2)
    g.init_iframe()
    g.build_grid()
    g.synchronize()
    res = {"n": n, "grid_dim": G, "live": int(g.live_count()), "reps": a.reps, "warmup": a.warmup}

    def call(fn, spec):
        return lambda: fn(g.h, C.byref(spec)) == 0 or sys.exit("the call failed: " + g.lib.psamd_last_error(g.h).decode())
    rec = torch.zeros(C.sizeof(ps.DepositResult), dtype=torch.uint8, device=dev)
    for k in (1, 2, 4):
        first, r = g.deposit(k, result=True)
        again = g.deposit(k)
        assert torch.equal(first.view(torch.int32), again.view(torch.int32)), "two deposits of one frame differ"
        total = float(first.double().sum().item())
        assert abs(total - r["mass"]) <= 1e-6 * r["mass"], (total, r)
        out = torch.empty_like(first)
        torch.cuda.synchronize()
        spec = ps.DepositSpec(refine=k, out=out.data_ptr(), capacity=out.numel(), result_dev=rec.data_ptr())
        res["refine_%d" % k] = dict(timed(g, call(g.lib.psamd_deposit, spec), a.reps, a.warmup), voxels=r["voxels"], bodies=r["bodies"],
                                    mass=r["mass"], vmax=r["vmax"])
    res["potential"] = timed(g, call(g.lib.psamd_potential, ps.Potential()), a.reps, a.warmup)
    g.calc_forces()
    g.synchronize()
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        f.write("psamd_deposit at N = 2^20 (default configuration, %d^3 cells, uniform cloud of 2^20 filled and stepped twice, %d live),\n"
                "one MI355X; written by scripts/deposit_cost.py.  All figures from one run on one built frame: host clock around the call\n"
                "plus psamd_synchronize, the stream idle before it, median of %d calls after %d warm-ups.  A deposit is two kernels (the\n"
                "gather: one wave per block of at most 2 x 2 x 2 voxels of a cell, over the cell's 27 lists; the result record);\n"
                "psamd_potential (the result alone, three kernels) on the same frame beside them.  Before the timing every refine's array\n"
                "came out the same bytes twice and added up to the mass of its record.\n\n" % (G, res["live"], a.reps, a.warmup))
        f.write("%-16s %10s %12s %10s %10s %14s\n" % ("call", "voxels", "median us", "min us", "max us", "x potential"))
        pot = res["potential"]["us_median"]
        for k in (1, 2, 4):
            r = res["refine_%d" % k]
            f.write("%-16s %10d %12.1f %10.1f %10.1f %14.2f\n" % ("deposit refine %d" % k, r["voxels"], r["us_median"], r["us_min"], r["us_max"], r["us_median"] / pot))
        r = res["potential"]
        f.write("%-16s %10s %12.1f %10.1f %10.1f %14.2f\n" % ("potential", "-", r["us_median"], r["us_min"], r["us_max"], 1.0))
        f.write("\n" + json.dumps(res, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
