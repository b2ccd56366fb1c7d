"""What psamd_probe costs beside the pair stage and psamd_potential of the same frames.

    python scripts/probe_cost.py [--reps R] [--out profiles/probe_cost.txt]

One MI355X, the default N = 2^20 uniform cloud (cutoff forces, the benchmark's cloud).  Every frame starts from the same
saved state (snapshot_restore) and is run through the stage calls -- init_iframe, build_grid, probe, potential,
calc_forces -- with timing on.  Two probe sets of 65 536 entries, ACC | PHI: the positions of 65 536 live particles (an
export's pos4, every 16th-odd entry of it so that the set spreads over the box), and a regular 64 x 32 x 32 grid of
nodes over the box.  The probe call and the potential call between HIP events on the context's stream (their launches
and the gaps between them); the `pairs` timer of the same frames from psamd_get_timing.  One warm-up frame, then the
median of R frames, with the smallest and the largest beside it."""
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

M = 65536

READING = """
How to read it.  65 536 probes cost about twice what psamd_potential takes for all 321 670 listed particles, for two
reasons.  (1) Lane fill: a wave walks a stencil for ALL its lanes and keeps the result of the lanes that belong to the
cell; with 65 536 probes over 4096 cells a cell holds 16 of them, so a wave of 64 serves four cells one after the other
and a quarter of its lanes are used in each walk.  The cost follows the number of (wave, distinct cell) walks, not the
number of probes: many probes per cell (a dense grid, every particle of a frame) fill the lanes, a few per cell do not.
(2) ACC | PHI walks every list twice, once by the force pass's exact pair form and once by the
potential's lighter one; ACC alone or PHI alone costs its own walk only.  The grid set is the cheaper one presumably because its
nodes fall 16 to a cell exactly while the particles' set spreads unevenly (more distinct cells per wave); that was not
taken apart further.  The host route the call replaces (download_particles, download_cellgrid, a sum on the host) was
not timed here.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_cost.txt"))
    a = ap.parse_args()
    n = 1 << 20
    dev = torch.device("cuda", 0)
    g = ps.ParticleSystem(ps.default_config(device=0))
    g.fill_particles(g.uniform_cloud(n, 12345), age=np.float32(2.0), fert_age=np.float32(1e6))
    g.step(2)
    g.synchronize()
    g.snapshot_save()
    g.init_iframe()
    g.build_grid()
    pos = g.export_live(ps.EXPORT_POS)["pos4"]
    live = len(pos)
    stride = max(1, live // M)
    on_particles = pos[::stride][:M].contiguous()
    half = g.sizes.grid_dim * float(g.cfg.cell_size) / 2.0
    ax = [torch.linspace(-half, half, k + 1, device=dev)[:-1] + half / k for k in (64, 32, 32)]      # the nodes' cells' centres
    X, Y, Z = torch.meshgrid(*ax, indexing="ij")
    on_grid = torch.stack([X.ravel(), Y.ravel(), Z.ravel(), torch.zeros(M, device=dev)], 1).float().contiguous()
    first = {k: g.probe(p) for k, p in (("particles", on_particles), ("grid", on_grid))}
    g.calc_forces()
    stream = torch.cuda.ExternalStream(g.stream(), device=dev)
    out4 = torch.zeros((M, 4), dtype=torch.float32, device=dev)
    rec = torch.zeros(64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    specs = {k: ps.ProbeSpec(fields=ps.PROBE_ACC | ps.PROBE_PHI, max_count=M, pos4=p.data_ptr(), out4=out4.data_ptr(), result_dev=rec.data_ptr())
             for k, p in (("particles", on_particles), ("grid", on_grid))}
    pot = ps.Potential(result_dev=rec.data_ptr())
    us = {"particles": [], "grid": [], "potential": []}
    g.set_timing(True)
    for rep in range(a.reps + 1):
        g.snapshot_restore()
        g.init_iframe()
        g.build_grid()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record(stream)
        assert g.lib.psamd_probe(g.h, C.byref(specs["particles"])) == 0
        ev[1].record(stream)
        assert g.lib.psamd_probe(g.h, C.byref(specs["grid"])) == 0
        ev[2].record(stream)
        assert g.lib.psamd_potential(g.h, C.byref(pot)) == 0
        ev[3].record(stream)
        g.calc_forces()
        ev[3].synchronize()
        if rep:                                              # (the first frame warms the code objects up)
            for k, name in enumerate(("particles", "grid", "potential")):
                us[name].append(ev[k].elapsed_time(ev[k + 1]) * 1e3)
    g.synchronize()
    t, launches = g.timing()
    g.close()
    res = {"n": n, "live": live, "probes": M, "reps": a.reps, "pairs_timer_us_per_frame": t["pairs"] / max(launches, 1),
           "served": {k: int(v["served"]) for k, v in first.items()}, "nonfinite": {k: int(v["nonfinite"]) for k, v in first.items()}}
    for k, v in us.items():
        res[k + "_us"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    with open(a.out, "w") as f:
        f.write("psamd_probe (ACC | PHI, 65 536 entries) beside psamd_potential and the pair stage of the same frames, one MI355X,\n"
                "N = 2^20 uniform cloud filled and stepped twice (%d live), every frame from that saved state (snapshot_restore)\n"
                "and run through the stage calls (init_iframe, build_grid, probe, probe, potential, calc_forces).\n"
                "probe / potential: HIP events on the context's stream around the call (its launches and their gaps), one warm-up\n"
                "frame, then %d frames: median (min .. max).  pairs: the timer of psamd_get_timing over the same frames.  us.\n\n" % (live, a.reps))
        for name, key in (("probe, 65 536 on particles' own positions", "particles_us"), ("probe, 65 536 on a regular grid", "grid_us"),
                          ("psamd_potential (result only)", "potential_us")):
            v = res[key]
            f.write("%-44s %10.1f   (%.1f .. %.1f)\n" % (name, v["median"], v["min"], v["max"]))
        f.write("%-44s %10.1f\n" % ("pairs timer, per frame", res["pairs_timer_us_per_frame"]))
        f.write(READING)
        f.write("\n" + json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
