"""Cost of psamd_knn on the benchmark frame (N = 2^20 on 16^3 cells, two steps in) for k = 1, 8 and 32 at radius 1.0 and at
cell_size, beside psamd_neighbours' count-and-offsets call and its with-lists call on the same frame in the same run: a host
clock around the call plus psamd_synchronize, the stream idle before it, after the first call has allocated (the protocol of
profiles/groups_cost.txt).  The with-lists time is the figure to beat at every k -- today's route is that call plus a ragged
sort; the count-and-offsets time is what k = 1 should be close to: the same walk with the same work per candidate.  Prints the
lines profiles/knn_cost.txt holds."""
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
    count = torch.zeros(live, dtype=torch.int32, device=dev)
    offs = torch.zeros(live + 1, dtype=torch.int64, device=dev)
    found = torch.zeros(live, dtype=torch.int32, device=dev)
    who = torch.zeros(live * ps.KNN_MAX_K, dtype=torch.int32, device=dev)
    d2 = torch.zeros(live * ps.KNN_MAX_K, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    for radius in (1.0, cs):
        wanted = g.neighbours(radius, lists=False)["wanted"]      # (the first calls allocate)
        lst = torch.zeros(max(wanted, 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        counts = ps.NeighboursSpec(radius=radius, count=count.data_ptr(), offsets=offs.data_ptr(), capacity=live)
        lists = ps.NeighboursSpec(radius=radius, count=count.data_ptr(), offsets=offs.data_ptr(), capacity=live, list=lst.data_ptr(), list_capacity=wanted)
        a = timed(g, lambda: g.lib.psamd_neighbours(g.h, C.byref(counts)))
        b = timed(g, lambda: g.lib.psamd_neighbours(g.h, C.byref(lists)))
        print("radius %-4g neighbours: wanted %9d | count and offsets %.3f ms (min %.3f) | with the lists %.3f ms (min %.3f)" % (radius, wanted, a[0], a[1], b[0], b[1]))
        for k in (1, 8, 32):
            rec = g.knn(radius, k, capacity=0)
            record = ps.KnnSpec(radius=radius, k=k)
            rows = ps.KnnSpec(radius=radius, k=k, found=found.data_ptr(), who=who.data_ptr(), d2=d2.data_ptr(), capacity=live)
            c = timed(g, lambda: g.lib.psamd_knn(g.h, C.byref(record)))
            d = timed(g, lambda: g.lib.psamd_knn(g.h, C.byref(rows)))
            print("radius %-4g knn k = %2d: found %9d  full %7d of %d | record only %.3f ms (min %.3f) | found + rows %.3f ms (min %.3f)"
                  % (radius, k, rec["found_sum"], rec["full"], rec["listed"], c[0], c[1], d[0], d[1]))
        del lst
    g.calc_forces()
    g.synchronize()
    g.close()


if __name__ == "__main__":
    sys.exit(main())
