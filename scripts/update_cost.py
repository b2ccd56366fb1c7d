"""What psamd_update costs, mid-run, on the default N = 2^20 uniform cloud (one MI355X).

    python scripts/update_cost.py [--reps R] [--warmup W] [--out profiles/update_cost.txt]

In one run, on one context: a kick (VEL | ADD) of 65 536 distinct live ids in random order by id; a kick of every live
particle by export order; beside them psamd_export_live of VEL, the streaming pass over the same field that was there
before; and the host route a caller had to take before psamd_update -- download_particles, the same addition in numpy,
upload_particles -- on a twin context.  Every figure is a host clock around the call plus psamd_synchronize, with an idle
stream before it, after warm-up calls.  The first repetitions check that the kick by id, the kick by export order of
the same entries and the host route leave the same particle bytes."""
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

COUNT = 65536


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
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_cost.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = 1 << 20
    cfg = ps.default_config(device=0)
    g, twin = ps.ParticleSystem(cfg), ps.ParticleSystem(cfg)
    xyz = g.uniform_cloud(n, 12345)
    for s in (g, twin):
        s.fill_particles(xyz, age=np.float32(2.0), fert_age=np.float32(1e6))
        s.step(2)
        s.synchronize()
        s.snapshot_save()
    ex = g.export_live(ps.EXPORT_ID)
    eid = ex["id"].cpu().numpy()
    live = int(ex["count"])
    rng = np.random.default_rng(7)
    ids_host = rng.permutation(eid)[:COUNT].astype(np.int32)
    kick_host = np.ascontiguousarray(np.concatenate([rng.uniform(-1, 1, (live, 3)), np.zeros((live, 1))], 1).astype(np.float32))
    ids = torch.from_numpy(ids_host).to(dev)
    kick = torch.from_numpy(kick_host).to(dev)
    out_vel = torch.empty((g.owned_slots(), 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    by_id = ps.Update(fields=ps.UPDATE_VEL | ps.UPDATE_ADD, max_count=COUNT, ids=ids.data_ptr(), vel4=kick.data_ptr())
    by_order = ps.Update(fields=ps.UPDATE_VEL | ps.UPDATE_ADD | ps.UPDATE_EXPORT_ORDER, max_count=live, vel4=kick.data_ptr())
    export = ps.Export(fields=ps.EXPORT_VEL, capacity=g.owned_slots(), vel4=out_vel.data_ptr())
    res = {"n": n, "slots": g.owned_slots(), "live": live, "reps": a.reps, "warmup": a.warmup}

    def call(fn, spec):
        return lambda: fn(g.h, C.byref(spec)) == 0 or sys.exit("the call failed: " + g.lib.psamd_last_error(g.h).decode())
    # the three routes leave the same bytes: the first COUNT particles of the export, kicked by id, by export order, on the host
    g.snapshot_restore()
    first_ids = torch.from_numpy(eid[:COUNT].copy()).to(dev)
    first = ps.Update(fields=ps.UPDATE_VEL | ps.UPDATE_ADD, max_count=COUNT, ids=first_ids.data_ptr(), vel4=kick.data_ptr())
    torch.cuda.synchronize()
    call(g.lib.psamd_update, first)()
    after_id = g.download_particles()
    assert g.update_result()["updated"] == COUNT
    g.snapshot_restore()
    first.ids, first.fields = None, first.fields | ps.UPDATE_EXPORT_ORDER
    call(g.lib.psamd_update, first)()
    assert g.update_result()["updated"] == COUNT
    assert g.download_particles().tobytes() == after_id.tobytes(), "by id and by export order left different bytes"
    g.snapshot_restore()
    # (the kicks add up over the repetitions: the velocities drift, the work does not change)
    res["by_id"] = dict(timed(g, call(g.lib.psamd_update, by_id), a.reps, a.warmup), entries=COUNT)
    assert g.update_result()["updated"] == COUNT
    res["by_export_order"] = dict(timed(g, call(g.lib.psamd_update, by_order), a.reps, a.warmup), entries=live)
    assert g.update_result()["updated"] == live
    res["export_live_vel"] = dict(timed(g, call(g.lib.psamd_export_live, export), a.reps, a.warmup), entries=live)
    host_us, parts = [], None
    for rep in range(a.host_reps):
        twin.snapshot_restore()
        twin.synchronize()
        t0 = time.perf_counter()
        p = twin.download_particles()
        t1 = time.perf_counter()
        sel = eid[:COUNT]
        for k, f in enumerate(("vx", "vy", "vz")):
            p[f][sel] = p[f][sel] + kick_host[:COUNT, k]
        t2 = time.perf_counter()
        twin.upload_particles(p)
        twin.synchronize()
        t3 = time.perf_counter()
        host_us.append((t3 - t0) * 1e6)
        parts = {"download_us": (t1 - t0) * 1e6, "edit_us": (t2 - t1) * 1e6, "upload_us": (t3 - t2) * 1e6}
        if rep == 0:
            assert twin.download_particles().tobytes() == after_id.tobytes(), "the host route and psamd_update left different bytes"
    res["host_route"] = dict({"us_median": float(np.median(host_us)), "us_min": float(np.min(host_us)), "reps": a.host_reps, "entries": COUNT},
                             **{"last_" + k: v for k, v in parts.items()})
    # the bytes the export-order kick has to move: the cell word of every owned slot twice, a float4 read and written per
    # live particle, a float4 read per entry
    moved = 2 * 4 * res["slots"] + 3 * 16 * live
    res["by_export_order"]["bytes_moved"] = moved
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        f.write("psamd_update at N = 2^20 (default configuration, uniform cloud of 2^20 filled and stepped twice, %d owned slots,\n"
                "%d live), one MI355X; written by scripts/update_cost.py.  All figures from one run, on one context: host clock\n"
                "around the call plus psamd_synchronize, the stream idle before it, median of %d calls after %d warm-ups.\n"
                "by id: a kick (VEL | ADD) of 65 536 distinct live ids in random order (a memset and three kernels); by export order: a\n"
                "kick of every live particle (two kernels); export_live: psamd_export_live of VEL on the same context (two kernels),\n"
                "the streaming pass over the same field that was there before; host route: download_particles, the addition for 65 536\n"
                "particles in numpy, upload_particles on a twin context, median of %d.  Before the timing the kick by id, the kick by\n"
                "export order of the same entries and the host route were checked to leave the same particle bytes.\n\n"
                % (res["slots"], res["live"], a.reps, a.warmup, a.host_reps))
        f.write("%-18s %10s %12s %10s %10s\n" % ("route", "entries", "median us", "min us", "max us"))
        for key, name in (("by_id", "by id"), ("by_export_order", "by export order"), ("export_live_vel", "export_live VEL")):
            r = res[key]
            f.write("%-18s %10d %12.1f %10.1f %10.1f\n" % (name, r["entries"], r["us_median"], r["us_min"], r["us_max"]))
        r = res["host_route"]
        f.write("%-18s %10d %12.1f %10.1f\n" % ("host route", r["entries"], r["us_median"], r["us_min"]))
        ratio = res["by_export_order"]["us_median"] / res["export_live_vel"]["us_median"]
        f.write("\nby export order / export_live VEL: %.2f.  The kick moves %.1f MB (the cell word of every owned slot in both kernels, per\n"
                "live particle a float4 of the entries read and a float4 of vel4 read and written): %.0f GB/s over the median, synchronize\n"
                "and two launches included; the export reads cell, pos4 and vel4 in its count pass (its statistics) and vel4 again in its\n"
                "write pass.\n" % (ratio, moved / 1e6, moved / res["by_export_order"]["us_median"] / 1e3))
        f.write("\n" + json.dumps(res, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
