"""What psamd_inject costs against psamd_fill_particles, mid-run, on the default N = 2^20 uniform cloud (one MI355X).

    python scripts/inject_cost.py [--reps R] [--out profiles/inject_cost.txt] [--kernel-stats DIR]

For each batch of 1 024, 65 536 and 262 144 uniform entries: the inject's kernel time per call (HIP events on the
context's stream around the call), and fill_particles of the same batch on a twin context (a host clock around the
call).  Both start from the same saved state (snapshot_restore before every call, outside the timed span), where the
host's queue mirror is stale as it is after a step: fill pulls the queues, places, and pushes them back.  The first
call of each size also checks that both leave the same bytes.
--kernel-stats DIR: a directory rocprofv3 --kernel-trace --stats wrote (a run of its own, e.g. with --reps 5
--no-fill); its *kernel_stats.csv rows of the inject kernels are appended to the report."""
import argparse
import ctypes as C
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime)

import particlesystem_amd as ps  # noqa: E402

SIZES = (1024, 65536, 262144)


def entries(g, n, seed, dev):
    rng = np.random.default_rng(seed)
    xyz = g.uniform_cloud(n, seed)
    pos4 = np.concatenate([xyz, rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)], 1)
    vel4 = np.concatenate([rng.uniform(-20, 20, (n, 3)), rng.uniform(0.0, 9.0, (n, 1))], 1).astype(np.float32)
    fert = rng.uniform(3.0, 12.0, n).astype(np.float32)
    host = (np.ascontiguousarray(pos4), np.ascontiguousarray(vel4), fert)
    return host, tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in host)


def kernel_rows(d):
    """(kernel, entries) -> durations in us, from the rocpd database(s) rocprofv3 wrote under d"""
    import sqlite3
    out = {}
    for path in glob.glob(os.path.join(d, "**", "*.db"), recursive=True):
        con = sqlite3.connect(path)
        for name, grid, dur in con.execute("select name, grid_x, duration from kernels where name like '%inject%'"):
            short = name.split("(")[0].replace("void ", "").replace("psamd::", "")
            out.setdefault((short, int(grid)), []).append(dur / 1e3)
        con.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-fill", action="store_true", help="inject only (the profiler's run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inject_cost.txt"))
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        rows = kernel_rows(a.kernel_stats)
        order = ("k_inject_locate<true>", "k_inject_scan", "k_inject_fail", "k_inject_place", "k_inject_commit")
        with open(a.out, "a") as f:
            f.write("\nrocprofv3 --kernel-trace --stats, a run of its own (inject only, --reps 5 per size): median kernel durations, us\n")
            f.write("(grid: threads launched; k_inject_locate has one workgroup of 1024 threads per tile of 4096 entries, the\n"
                    " one-workgroup kernels k_inject_scan and k_inject_commit are sized by the records, not the entries)\n")
            for name in order:
                for (k, grid), d in sorted(rows.items(), key=lambda kv: kv[0][1]):
                    if k == name:
                        f.write("  %-24s grid %8d  calls %3d  median %8.2f  min %8.2f  max %8.2f\n"
                                % (k, grid, len(d), float(np.median(d)), min(d), max(d)))
        print("appended %d kernel groups to %s" % (len(rows), a.out))
        return
    dev = torch.device("cuda", 0)
    n = 1 << 20
    cfg = ps.default_config(device=0)
    g = ps.ParticleSystem(cfg)
    twin = None if a.no_fill else ps.ParticleSystem(cfg)
    xyz = g.uniform_cloud(n, 12345)
    for s in [g] + ([twin] if twin else []):
        s.fill_particles(xyz, age=np.float32(2.0), fert_age=np.float32(1e6))
        s.step(2)
        s.synchronize()
        s.snapshot_save()
    stream = torch.cuda.ExternalStream(g.stream(), device=dev)
    res = {"n": n, "slots": g.owned_slots(), "reps": a.reps, "sizes": {}}
    for size in SIZES:
        host, (pos4, vel4, fert) = entries(g, size, 100 + size, dev)
        torch.cuda.synchronize()
        spec = ps.Inject(max_count=size, pos4=pos4.data_ptr(), vel4=vel4.data_ptr(), fert_age=fert.data_ptr())
        ev_us, fill_us = [], []
        for rep in range(a.reps):
            g.snapshot_restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert g.lib.psamd_inject(g.h, C.byref(spec)) == 0
            e1.record(stream)
            e1.synchronize()
            ev_us.append(e0.elapsed_time(e1) * 1e3)
            r = g.inject_result()
            assert r == {"done": size, "placed": size, "status": 0}, r
            if twin is None:
                continue
            twin.snapshot_restore()
            twin.synchronize()
            t0 = time.perf_counter()
            ids = twin.fill_particles(host[0][:, :3], age=host[1][:, 3], fert_age=host[2], w=host[0][:, 3], vxyz=host[1][:, :3])
            fill_us.append((time.perf_counter() - t0) * 1e6)
            if rep == 0:
                same = (g.download_particles().tobytes() == twin.download_particles().tobytes()
                        and all(x.tobytes() == y.tobytes() for x, y in zip(g.download_queues(), twin.download_queues())))
                assert same and len(ids) == size, "inject and fill left different bytes at %d entries" % size
        res["sizes"][size] = {"inject_us_event_median": float(np.median(ev_us)), "inject_us_event_min": float(np.min(ev_us)),
                              "inject_us_event_max": float(np.max(ev_us))}
        if fill_us:
            res["sizes"][size].update({"fill_us_host_median": float(np.median(fill_us)), "fill_us_host_min": float(np.min(fill_us)),
                                       "fill_same_bytes_as_inject": True})
    print(json.dumps(res, indent=1))
    if a.no_fill:
        return
    with open(a.out, "w") as f:
        f.write("psamd_inject against psamd_fill_particles at N = 2^20 (default configuration, uniform cloud of 2^20 filled and\n"
                "stepped twice, %d owned slots), one MI355X.  Batches of uniform entries (pos4, vel4, fert_age all given).\n"
                "Every call starts from the same saved state (snapshot_restore, outside the timed span); after a restore the\n"
                "host's queue mirror is stale, as after a step, so fill pulls and pushes the queues as it does mid-run.\n"
                "inject: HIP events on the context's stream around the call (the five kernels and their launch gaps), %d calls.\n"
                "fill: host clock around fill_particles of the same batch on a twin context, %d calls.  The first call of each\n"
                "size checked that both leave the same particle and queue bytes.\n\n" % (res["slots"], a.reps, a.reps))
        f.write("%10s %18s %14s %18s %10s\n" % ("entries", "inject med us", "inject min", "fill med us", "ratio"))
        for size in SIZES:
            s = res["sizes"][size]
            f.write("%10d %18.1f %14.1f %18.1f %10.0f\n" % (size, s["inject_us_event_median"], s["inject_us_event_min"],
                                                           s["fill_us_host_median"], s["fill_us_host_median"] / s["inject_us_event_median"]))
        f.write("\n" + json.dumps(res, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
