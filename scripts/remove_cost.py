"""What psamd_remove costs against the host route, mid-run, on the default N = 2^20 uniform cloud (one MI355X).

    python scripts/remove_cost.py [--reps R] [--warmup W] [--out profiles/remove_cost.txt]

By id: 65 536 distinct live ids in random order.  By box: a slab of the box in x, its width chosen on the host so that it
holds 65 536 live particles.  Both are timed with HIP events on the context's stream around the call (its four kernels
and their launch gaps); every repetition starts from the same saved state (snapshot_restore, outside the timed span).
The host route -- what a caller had to do before psamd_remove -- removes the same 65 536 ids on a twin context:
download_particles, download_queues, the reset + q_insert of every id in numpy (tests/remove_model.py's closed form; a
host clock around all of it), upload_particles, upload_queues.  The first repetition checks that all three leave the
same particle and queue bytes."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime)

import particlesystem_amd as ps  # noqa: E402
import remove_model as M  # noqa: E402

COUNT = 65536


def state(g):
    return (g.download_particles(),) + tuple(g.download_queues())


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remove_cost.txt"))
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
    ex = g.export_live(ps.EXPORT_POS | ps.EXPORT_ID)
    pos, eid = ex["pos4"].cpu().numpy(), ex["id"].cpu().numpy()
    rng = np.random.default_rng(7)
    ids_host = rng.permutation(eid)[:COUNT].astype(np.int32)
    ids = torch.from_numpy(ids_host).to(dev)
    xs = np.sort(pos[:, 0])
    lo = (float(xs[0]), -1e30, -1e30)
    hi = (float(xs[COUNT]), 1e30, 1e30)
    box_ids = eid[(pos[:, 0] >= np.float32(lo[0])) & (pos[:, 0] < np.float32(hi[0]))]
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(g.stream(), device=dev)
    by_id = ps.Remove(max_count=COUNT, ids=ids.data_ptr())
    by_box = ps.Remove(flags=ps.REMOVE_BOX)
    for k in range(3):
        by_box.lo[k], by_box.hi[k] = lo[k], hi[k]
    res = {"n": n, "slots": g.owned_slots(), "live": int(ex["count"]), "reps": a.reps, "warmup": a.warmup}
    after = {}
    for name, spec, want in (("by_id", by_id, COUNT), ("by_box", by_box, len(box_ids))):
        us = []
        for rep in range(a.warmup + a.reps):
            g.snapshot_restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert g.lib.psamd_remove(g.h, C.byref(spec)) == 0
            e1.record(stream)
            e1.synchronize()
            if rep >= a.warmup:
                us.append(e0.elapsed_time(e1) * 1e3)
            r = g.remove_result()
            assert r["removed"] == want and r["dropped"] == 0, r
        after[name] = state(g)
        res[name] = {"selected": want, "us_event_median": float(np.median(us)), "us_event_min": float(np.min(us)),
                     "us_event_max": float(np.max(us))}
    # the host route on the twin, and what the by-box selection gives through by id
    host_us, parts = [], None
    sizes = twin.sizes
    for rep in range(a.host_reps):
        twin.snapshot_restore()
        twin.synchronize()
        t0 = time.perf_counter()
        p = twin.download_particles()
        qi, q = twin.download_queues()
        t1 = time.perf_counter()
        p2, qi2, q2, _, r = M.closed_form(sizes, sizes.num_cells, p, qi, q, ids_host)
        t2 = time.perf_counter()
        twin.upload_particles(p2)
        twin.upload_queues(qi2, q2)
        twin.synchronize()
        t3 = time.perf_counter()
        host_us.append((t3 - t0) * 1e6)
        parts = {"download_us": (t1 - t0) * 1e6, "edit_us": (t2 - t1) * 1e6, "upload_us": (t3 - t2) * 1e6}
        assert r["removed"] == COUNT
        if rep == 0:
            assert same(state(twin), after["by_id"]), "the host route and psamd_remove by id left different bytes"
            twin.snapshot_restore()
            assert twin.remove(ids=torch.from_numpy(box_ids.astype(np.int32)).to(dev))["removed"] == len(box_ids)
            assert same(state(twin), after["by_box"]), "by box and by id of the same selection left different bytes"
    res["host_route"] = dict({"us_host_median": float(np.median(host_us)), "us_host_min": float(np.min(host_us)), "reps": a.host_reps},
                             **{"last_" + k: v for k, v in parts.items()})
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        f.write("psamd_remove against the host route at N = 2^20 (default configuration, uniform cloud of 2^20 filled and stepped\n"
                "twice, %d owned slots, %d live), one MI355X; written by scripts/remove_cost.py.\n"
                "Every call starts from the same saved state (snapshot_restore, outside the timed span).\n"
                "by id: 65 536 distinct live ids in random order; by box: a slab in x that holds %d live particles.  HIP events on\n"
                "the context's stream around the call (four kernels and their launch gaps), median of %d calls after %d warm-ups.\n"
                "host route: download_particles, download_queues, reset + q_insert of the same 65 536 ids in numpy, upload_particles,\n"
                "upload_queues on a twin context; host clock, median of %d.  The first repetition checked that the host route and\n"
                "by id, and by box and by id of the box's selection, leave the same particle and queue bytes.\n\n"
                % (res["slots"], res["live"], res["by_box"]["selected"], a.reps, a.warmup, a.host_reps))
        f.write("%-12s %12s %14s %12s\n" % ("route", "removed", "median us", "min us"))
        f.write("%-12s %12d %14.1f %12.1f\n" % ("by id", COUNT, res["by_id"]["us_event_median"], res["by_id"]["us_event_min"]))
        f.write("%-12s %12d %14.1f %12.1f\n" % ("by box", res["by_box"]["selected"], res["by_box"]["us_event_median"], res["by_box"]["us_event_min"]))
        f.write("%-12s %12d %14.1f %12.1f\n" % ("host route", COUNT, res["host_route"]["us_host_median"], res["host_route"]["us_host_min"]))
        f.write("\n" + json.dumps(res, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
