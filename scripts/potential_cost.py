"""What psamd_potential costs beside the pair stage of the same frames, and how well the energy it completes is kept.

    python scripts/potential_cost.py [--reps R] [--out profiles/potential_cost.txt] [--no-drift]

Two configurations on one MI355X: the default N = 2^20 uniform cloud (cutoff forces) and the all-pairs N = 2^18 cloud
(BASELINE configs[1]).  Every frame starts from the same saved state (snapshot_restore) and is run through the stage
calls -- init_iframe, build_grid, potential, calc_forces -- with timing on: the potential call between HIP events on the context's stream (its launches and their
gaps), the `collide` and `pairs` timers of the same frames from psamd_get_timing.  The first frame's phi and U are
compared with an fp64 direct sum on a sample (the accuracy tests are tests/test_gpu_potential.py; this is the record),
and the work of the two passes is counted from the frame's lists: the potential pass serves every listed particle, the
force pass those that need a force (psamd_download_force_counts), each over the same bodies.

Then the energy drift of a small all-pairs cloud (4096 particles, collision radius 0, at rest at the start) over 200
steps, for the default update and for PSAMD_FLAG_EULER, at dt and dt / 2: information, asserted nowhere."""
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

CONFIGS = (("cutoff N = 2^20 (default constants)", 1 << 20, {}),
           ("all-pairs N = 2^18", 1 << 18, {"max_particles_num": 1 << 18, "flags": ps.FLAG_ALL_PAIRS}))


READING = """
How to read it.  The call takes longer than the `pairs` timer of its frame in both configurations, for two reasons the
table shows.  (1) It serves more particles: every listed one, where the force pass serves those that need a force
(neither collided this step nor a kid) -- 14 times as many on the cutoff frame, 1.9 times on the all-pairs frame -- over
the same bodies each; the cutoff frame's force pass is mostly fixed cost at that size.  (2) Per pair it is no faster than
the exact force pass, although a pair costs it fewer instructions: its waves are (cell, 64-particle slice) tasks, so the
last slice of every cell is partly empty (lane fill 0.63 and 0.50 here), where the force pass balances its waves over
the stencil steps and packs partly filled slices, and the all-pairs far pass takes dense tasks of 64 particles whatever
their cells.  Per occupied lane the potential pass is the cheaper one (pairs/s divided by the lane fill).  Dense tasks for
the potential pass would need the per-lane stencil exclusion of k_allp_far and are not part of this change.
"""


def sample_error(g, phi, ids, all_pairs, m=256):
    """largest relative error of phi over m particles against an fp64 direct sum of the frame's bodies"""
    p, cg = g.download_particles(), g.download_cellgrid()
    G, eps2 = g.sizes.grid_dim, float(g.cfg.eps2)
    xyz = np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float64)
    w = np.where(p["age"] < g.cfg.life_steps * g.cfg.dt / 10.0, 0.0, p["w"].astype(np.float64))
    count, lists = cg[:, 0], cg[:, 1:]
    everybody = np.concatenate([lists[c, :count[c]] for c in np.nonzero(count)[0]])
    full = np.full(len(p), np.nan, np.float32)
    full[ids] = phi
    worst = 0.0
    for i in np.random.default_rng(1).choice(everybody, m, replace=False):
        if all_pairs:
            js = everybody
        else:
            c = int(p["cell"][i])
            i3, r = divmod(c, G * G)
            i1, i2 = divmod(r, G)
            js = np.concatenate([lists[n, :count[n]] for n in
                                 [((i3 + a) * G + i1 + b) * G + i2 + d for a in (-1, 0, 1) for b in (-1, 0, 1) for d in (-1, 0, 1)
                                  if 0 <= i3 + a < G and 0 <= i1 + b < G and 0 <= i2 + d < G]])
        js = js[js != i]
        d = xyz[js] - xyz[i]
        ref = -float((w[js] / np.sqrt((d * d).sum(1) + eps2)).sum())
        worst = max(worst, abs(float(full[i]) - ref) / abs(ref))
    return worst


def work(g):
    """of the built frame whose pair stage has run: particles and pairs of the potential pass and of the force pass, and how
    full the potential pass's 64-lane (cell, slice) tasks are"""
    G = g.sizes.grid_dim
    count = g.download_cellgrid()[:, 0].astype(np.int64).reshape(G, G, G)
    force = g.download_force_counts().astype(np.int64).reshape(G, G, G)
    if g.cfg.flags & ps.FLAG_ALL_PAIRS:
        bodies = np.full_like(count, count.sum())
    else:
        pad = np.pad(count, 1)
        bodies = sum(pad[1 + a:1 + a + G, 1 + b:1 + b + G, 1 + c:1 + c + G] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1))
    return {"listed": int(count.sum()), "need_a_force": int(force.sum()), "potential_pairs": int((count * bodies).sum()),
            "force_pairs": int((force * bodies).sum()), "potential_lane_fill": float(count.sum() / (64.0 * ((count + 63) // 64).sum()))}


def cost(name, n, over, reps):
    dev = torch.device("cuda", 0)
    g = ps.ParticleSystem(ps.default_config(device=0, **over))
    g.fill_particles(g.uniform_cloud(n, 12345), age=np.float32(2.0), fert_age=np.float32(1e6))
    g.step(2)
    g.synchronize()
    g.snapshot_save()
    stream = torch.cuda.ExternalStream(g.stream(), device=dev)
    phi = torch.empty(g.owned_slots(), dtype=torch.float32, device=dev)
    rec = torch.zeros(C.sizeof(ps.PotentialResult), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with_phi = ps.Potential(phi=phi.data_ptr(), capacity=g.owned_slots(), result_dev=rec.data_ptr())
    alone = ps.Potential(result_dev=rec.data_ptr())
    out = {"n": n, "reps": reps}
    for label, spec in (("potential_with_phi_us", with_phi), ("potential_result_only_us", alone)):
        g.set_timing(True)
        us = []
        for rep in range(reps + 1):
            g.snapshot_restore()
            g.init_iframe()
            g.build_grid()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            assert g.lib.psamd_potential(g.h, C.byref(spec)) == 0
            e1.record(stream)
            g.calc_forces()
            e1.synchronize()
            if rep:                                          # (the first frame warms the code objects up)
                us.append(e0.elapsed_time(e1) * 1e3)
            elif "accuracy" not in out:
                g.snapshot_restore()
                g.init_iframe()
                g.build_grid()
                r = g.potential(phi=True)
                ids = g.export_live(ps.EXPORT_ID)["id"].cpu().numpy()
                out["accuracy"] = {"phi_max_rel_err_sample": sample_error(g, r["phi"].cpu().numpy(), ids, bool(over.get("flags", 0))),
                                   "potential": r["potential"], "listed": r["listed"]}
                g.calc_forces_pairs()
                out["work"] = work(g)
                g.calc_forces_apply()
        g.synchronize()
        t, launches = g.timing()
        out[label] = {"median": float(np.median(us)), "min": float(np.min(us)), "max": float(np.max(us))}
        out[label.replace("potential", "pairs_timer").replace("_us", "_us_per_frame")] = t["pairs"] / max(launches, 1)
        out[label.replace("potential", "collide_timer").replace("_us", "_us_per_frame")] = t["collide"] / max(launches, 1)
        g.set_timing(False)
    g.close()
    print(name, json.dumps(out))
    return out


def drift(flags, dt, steps=200, n=4096):
    g = ps.ParticleSystem(ps.default_config(device=0, max_particles_num=1 << 18, flags=ps.FLAG_ALL_PAIRS | flags, dt=dt,
                                            collision_radius=0.0))
    rng = np.random.default_rng(3)
    g.fill_particles(rng.normal(0.0, 6.0, (n, 3)).clip(-30, 30).astype(np.float32), age=np.float32(2.0), fert_age=np.float32(1e6))
    e = []                                                   # (age 2 + 200 dt stays below PARTICLE_LIFE = 300 dt: nobody dies of age)
    for k in range(steps + 1):
        g.init_iframe()
        g.build_grid()
        e.append(g.energy())
        g.calc_forces()
    g.synchronize()
    live = g.live_count()
    g.close()
    tot = np.array([x["total"] for x in e])
    return {"dt": dt, "euler": bool(flags & ps.FLAG_EULER), "live_at_end": live, "E0": tot[0], "E_end": tot[-1],
            "kinetic_end": e[-1]["kinetic"], "potential_end": e[-1]["potential"],
            "max_rel_drift": float(np.max(np.abs(tot - tot[0])) / abs(tot[0])), "end_rel_drift": float((tot[-1] - tot[0]) / abs(tot[0]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-drift", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "potential_cost.txt"))
    a = ap.parse_args()
    res = {"cost": {name: cost(name, n, over, a.reps) for name, n, over in CONFIGS}}
    if not a.no_drift:
        dt = ps.default_config().dt
        res["drift"] = [drift(f, d) for f in (0, ps.FLAG_EULER) for d in (dt, dt / 2)]
    with open(a.out, "w") as f:
        f.write("psamd_potential beside the pair stage of the same frames, one MI355X; frames run through the stage calls\n"
                "(init_iframe, build_grid, potential, calc_forces), uniform cloud filled and stepped twice, every\n"
                "frame from that saved state (snapshot_restore).\n"
                "potential: HIP events on the context's stream around the call (its launches and their gaps), median of %d frames;\n"
                "collide / pairs: the timers of psamd_get_timing over the same frames, per frame (pairs = the force pass; in the\n"
                "all-pairs configuration it includes the far pass).  us.\n\n" % a.reps)
        f.write("%-38s %14s %14s %12s %12s %14s\n" % ("configuration", "potential+phi", "result only", "collide", "pairs", "phi err (smp)"))
        for name, c in res["cost"].items():
            f.write("%-38s %14.1f %14.1f %12.1f %12.1f %14.2g\n" % (name, c["potential_with_phi_us"]["median"], c["potential_result_only_us"]["median"],
                                                                 c["collide_timer_with_phi_us_per_frame"], c["pairs_timer_with_phi_us_per_frame"],
                                                                 c["accuracy"]["phi_max_rel_err_sample"]))
        f.write("\nThe work behind those times, from the frame's lists: the potential pass serves every listed particle (collided ones\n"
                "and kids too), the force pass the particles that need a force; both walk the same bodies per particle.\n"
                "lane fill: listed particles per lane of the potential pass's (cell, 64-particle slice) waves.\n\n")
        f.write("%-38s %10s %12s %14s %14s %16s %16s %10s\n" % ("configuration", "listed", "need force", "pot. pairs", "force pairs", "pot. Gpairs/s",
                                                                "force Gpairs/s", "lane fill"))
        for name, c in res["cost"].items():
            w = c["work"]
            f.write("%-38s %10d %12d %14.4g %14.4g %16.0f %16.0f %10.2f\n" % (
                name, w["listed"], w["need_a_force"], w["potential_pairs"], w["force_pairs"],
                w["potential_pairs"] / c["potential_result_only_us"]["median"] / 1e3,
                w["force_pairs"] / max(c["pairs_timer_with_phi_us_per_frame"], 1e-9) / 1e3, w["potential_lane_fill"]))
        f.write(READING)
        if "drift" in res:
            f.write("\nEnergy drift, information only: 4096 particles (normal cloud, sigma 6, at rest), all-pairs, collision radius 0,\n"
                    "200 steps; E = kinetic (psamd_live_stats) + potential (psamd_potential) at every frame.  The cloud collapses within\n"
                    "the run and the step's clamps (MAX_V, MAX_DX = one cell per step) do not conserve energy: this is a record, not a test.\n\n")
            f.write("%-10s %10s %16s %16s %14s %14s\n" % ("update", "dt", "E(0)", "E(200)", "max |dE|/|E0|", "dE(200)/|E0|"))
            for d in res["drift"]:
                f.write("%-10s %10.4g %16.8g %16.8g %14.3g %14.3g\n" % ("euler" if d["euler"] else "default", d["dt"], d["E0"], d["E_end"],
                                                                      d["max_rel_drift"], d["end_rel_drift"]))
        f.write("\n" + json.dumps(res, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
