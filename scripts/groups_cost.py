"""Cost of psamd_groups on the benchmark frame (N = 2^20 on 16^3 cells, two steps in), beside psamd_neighbours' count-and-offsets
call on the same frame in the same run: a host clock around the call plus psamd_synchronize, the stream idle before it, after
the first call has allocated (the protocol of profiles/deposit_cost.txt).  Prints the lines profiles/groups_cost.txt holds."""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime)

import particlesystem_amd as ps  # noqa: E402


def timed(g, fn, reps=20):
    out = []
    for _ in range(reps):
        g.synchronize()
        t = time.perf_counter()
        assert fn() == 0
        g.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out)


def main():
    n = 1 << 20
    dev = torch.device("cuda", 0)
    g = ps.ParticleSystem(ps.default_config(max_particles_num=n))
    g.fill_particles(g.uniform_cloud(n, 1), age=np.float32(3.0), fert_age=np.float32(1e6))
    g.step(2)
    g.init_iframe()
    g.build_grid()
    live, slots, cs = g.live_count(), g.owned_slots(), float(g.cfg.cell_size)
    print("N = %d on %d^3 cells, two steps in: %d live in %d owned slots" % (n, g.sizes.grid_dim, live, slots))
    count = torch.zeros(slots, dtype=torch.int32, device=dev)
    offs = torch.zeros(slots + 1, dtype=torch.int64, device=dev)
    group = torch.zeros(slots, dtype=torch.int32, device=dev)
    first = torch.zeros(slots, dtype=torch.int32, device=dev)
    size = torch.zeros(slots, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for radius in (0.4, 1.0, cs):
        g.neighbours(radius, lists=False)                     # (the first calls allocate)
        rec = g.groups(radius, group_capacity=0)
        assert rec["unfinished"] == 0, rec
        counts = ps.NeighboursSpec(radius=radius, count=count.data_ptr(), offsets=offs.data_ptr(), capacity=slots)
        record = ps.GroupsSpec(radius=radius)
        arrays = ps.GroupsSpec(radius=radius, group=group.data_ptr(), capacity=slots, group_first=first.data_ptr(), group_size=size.data_ptr(),
                               group_capacity=slots)
        a = timed(g, lambda: g.lib.psamd_groups(g.h, C.byref(record)))
        b = timed(g, lambda: g.lib.psamd_groups(g.h, C.byref(arrays)))
        c = timed(g, lambda: g.lib.psamd_neighbours(g.h, C.byref(counts)))
        print("radius %-4g members %8d  groups %8d  links %9d  largest %7d | record only %.3f ms (min %.3f) | group[] + tables %.3f ms (min %.3f) | "
              "neighbours' counts beside it %.3f ms (min %.3f)" % (radius, rec["members"], rec["groups"], rec["links"], rec["largest"], a[0], a[1], b[0], b[1], c[0], c[1]))
    g.calc_forces()
    g.synchronize()
    g.close()


if __name__ == "__main__":
    sys.exit(main())
