"""What psamd_export_live costs mid-run, on the default N = 2^20 uniform cloud (one MI355X).

    python scripts/export_cost.py [--steps S] [--warmup W] [--out FILE]

After each of S free-running steps: the export of POS | VEL | ID and the statistics into device arrays of the container's
size, timed with HIP events on the context's stream around the call (its two kernels and the launch gap).  The first
export is checked against download_live.  For the kernels one by one, run the script under
rocprofv3 --kernel-trace --stats (profiles/export_cost.txt was made so)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime)

import particlesystem_amd as ps  # noqa: E402

FIELDS = ps.EXPORT_POS | ps.EXPORT_VEL | ps.EXPORT_ID


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the report there")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = 1 << 20
    g = ps.ParticleSystem(ps.default_config(device=0))
    g.fill_particles(g.uniform_cloud(n, 12345), age=np.float32(2.0), fert_age=np.float32(1e6))
    slots = g.owned_slots()
    pos4, vel4 = (torch.empty((slots, 4), dtype=torch.float32, device=dev) for _ in range(2))
    ids = torch.empty(slots, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    stats = torch.zeros(C.sizeof(ps.LiveStats), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    spec = ps.Export(fields=FIELDS, capacity=slots, pos4=pos4.data_ptr(), vel4=vel4.data_ptr(), id=ids.data_ptr(),
                     count_dev=count.data_ptr(), stats_dev=stats.data_ptr())
    stream = torch.cuda.ExternalStream(g.stream(), device=dev)
    us, live = [], []
    for k in range(a.warmup + a.steps):
        g.step(1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        assert g.lib.psamd_export_live(g.h, C.byref(spec)) == 0
        e1.record(stream)
        e1.synchronize()
        if k == 0:
            want = g.download_live(FIELDS)
            m = int(count.item())
            assert m == want["count"] and np.array_equal(ids[:m].cpu().numpy(), want["id"]) \
                and pos4[:m].cpu().numpy().tobytes() == want["pos4"].tobytes(), "export_live and download_live differ"
        if k >= a.warmup:
            us.append(e0.elapsed_time(e1) * 1e3)
            live.append(int(count.item()))
    res = {"n": n, "slots": slots, "steps": a.steps, "warmup": a.warmup, "live_first": live[0], "live_last": live[-1],
           "export_us_event_median": float(np.median(us)), "export_us_event_min": float(np.min(us)), "export_us_event_max": float(np.max(us))}
    print(json.dumps(res, indent=1))
    if not a.out:
        return
    with open(a.out, "w") as f:
        f.write("psamd_export_live (POS | VEL | ID + statistics) at N = 2^20 (default configuration, uniform cloud of 2^20, %d owned\n"
                "slots), one MI355X; written by scripts/export_cost.py.  After each of %d free-running steps (%d warm-ups before): HIP\n"
                "events on the context's stream around the call (two kernels and their launch gap).  The first export was checked\n"
                "against download_live.\n\n" % (slots, a.steps, a.warmup))
        f.write("%-12s %14s %12s %12s\n" % ("live", "median us", "min us", "max us"))
        f.write("%-12s %14.1f %12.1f %12.1f\n" % ("%d..%d" % (live[0], live[-1]), res["export_us_event_median"], res["export_us_event_min"],
                                                 res["export_us_event_max"]))
        f.write("\n" + json.dumps(res, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
