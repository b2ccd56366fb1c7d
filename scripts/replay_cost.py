"""What the life-cycle tail costs: the `lifecycle` timer and the whole step at bench.py's workload, and the long road.

    python scripts/replay_cost.py [--label NAME] [--steps K]

One MI355X.  (1) bench.py's workload: N = 2^20 uniform cloud, seed 2026, default constants, T_DATA mirror off; after 5 warm
steps, K steps each from the same fill (snapshot_restore), ParticleSystem.set_timing(True, every_stage=True): a host clock
around psamd_step(1) + psamd_synchronize, and the `lifecycle` stage's own timer (k_ops_hist + k_ops_scatter +
k_replay_commit).  (2) the long road: tests/test_gpu_parity.py::test_long_operation_lists[big]'s scene, its third step
(a list beyond every instance, replay_long, the serial walk; long_road() restates that test's scene and must follow
it), K times from the state two steps have left, timed the same way.
Prints one line, `AB {...}`: per figure [median, lowest, highest] (ms; the timers in us).  For an A/B of two builds run it
in alternating processes with PSAMD_LIB pointing at the other build (profiles/replay_unified.txt)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: F401, E402  (before the library: one HIP runtime)

import particlesystem_amd as ps  # noqa: E402


def timed(g, steps):
    """`steps` times one step from the saved state: host ms of the step, the lifecycle timer's us"""
    g.set_timing(True, every_stage=True)
    ms, us = [], []
    for _ in range(steps):
        g.snapshot_restore()
        g.synchronize()
        before = g.timing()[0]["lifecycle"]
        t0 = time.perf_counter()
        g.step(1)
        g.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        us.append(g.timing()[0]["lifecycle"] - before)
    g.set_timing(False)
    return {"step_ms": [float(np.median(ms)), float(np.min(ms)), float(np.max(ms))],
            "lifecycle_us": [float(np.median(us)), float(np.min(us)), float(np.max(us))]}


def bench_workload(steps):
    n, seed = 1 << 20, 2026
    g = ps.ParticleSystem(ps.default_config(device=0))
    g.set_tdata_mirror(False)
    rng = np.random.default_rng(seed)
    life = 300.0 * g.cfg.dt
    g.fill_particles(g.uniform_cloud(n, seed), age=rng.uniform(life / 7.0, life / 2.0, n).astype(np.float32), fert_age=np.float32(1e6))
    g.snapshot_save()
    for _ in range(5):
        g.snapshot_restore(); g.step(1)
    g.synchronize()
    r = timed(g, steps)
    g.close()
    return r


def long_road(steps):
    rng = np.random.default_rng(121)
    blob = rng.uniform(-4.9, 4.9, (7200, 3)).astype(np.float32)
    outer = rng.uniform(-9.9, -0.1, (4800, 3)).astype(np.float32)
    outer = outer[~(outer > -5.0).all(axis=1)]
    rest = np.random.default_rng(122).uniform(-40.0, 40.0, (5000, 3)).astype(np.float32)
    rest = rest[(np.abs(rest) > 10.0).any(axis=1)]
    xyz = np.concatenate([blob, outer, rest])
    v = np.zeros_like(xyz)
    v[:len(blob) + len(outer)] = 300.0
    g = ps.ParticleSystem(ps.default_config(device=0, collision_radius=0.0, max_particles_num=1 << 21))
    g.fill_particles(xyz, age=np.float32(3.0), fert_age=np.float32(1e6), vxyz=v)
    g.step(2)
    g.synchronize()
    g.snapshot_save()
    r = timed(g, steps)
    r["max_ops_one_queue"] = int(g.counters["max_ops_one_queue"])
    r["relocations_lost"] = int(g.counters["relocations_lost"])
    g.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="build")
    ap.add_argument("--steps", type=int, default=40)
    a = ap.parse_args()
    print("AB " + json.dumps({"label": a.label, "bench": bench_workload(a.steps), "long_road": long_road(a.steps)}), flush=True)


if __name__ == "__main__":
    main()
