"""SHA-256 digests of what the far-field contexts compute on fixed small frames (PSAMD_FLAG_FAR_MONOPOLE, PSAMD_FLAG_FAR_PYRAMID):
the sorted order, the force records and an acceleration-and-potential probe with PSAMD_PROBE_FAR at 256 fixed points; for the
cases that run whole steps, the exported state after the third.

    python scripts/far_bits.py --commit <the commit the library was built from> [--out tests/golden/far_bits.json]

Only the public Python API is used, so the same file runs on any commit that has the two flags and the far probe.  The
committed tests/golden/far_bits.json was written on one MI355X at the commit it names; tests/test_gpu_far_bits.py recomputes
the digests with digests_of() and compares.  A digest that differs means that a refactor of the far walk changed an
association (or the sort, or the moments): the code is wrong then, not the file."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime)

import particlesystem_amd as ps  # noqa: E402

MONO, PYR, FAST, EXPL = ps.FLAG_FAR_MONOPOLE, ps.FLAG_FAR_PYRAMID, ps.FLAG_FAST_MATH, ps.FLAG_EXPLOSIONS
GRID = {6: dict(chunk_factor=2, chunk_dim=3), 8: dict(chunk_factor=2, chunk_dim=4), 10: dict(chunk_factor=2, chunk_dim=5),
        16: dict(chunk_factor=4, chunk_dim=4, x_factor=8)}      # (x_factor: lists of 40, for 4 a cell in the mean)
PROBES = 256

# name: (flags, G, bodies, whole steps)
CASES = {
    "flat-8-exact": (MONO, 8, 16 * 8 ** 3, 0),
    "flat-8-fast": (MONO | FAST, 8, 16 * 8 ** 3, 0),
    "flat-6-exact": (MONO, 6, 16 * 6 ** 3, 0),           # 216 cells: 4 blocks, the last one padded; parts without a block
    "pyramid-10-exact": (PYR, 10, 16 * 10 ** 3, 0),      # levels 10, 5, 3: odd sizes, clamped boxes
    "pyramid-10-fast": (PYR | FAST, 10, 16 * 10 ** 3, 0),
    "pyramid-16-exact": (PYR, 16, 4 * 16 ** 3, 0),       # a wave's 64 particles span many cells and several parents
    "flat-8-ragged": (MONO, 8, 5003, 0),                 # 4708 adults: the last dense task has 36 lanes
    "pyramid-8-ragged": (PYR, 8, 5003, 0),
    "flat-8-steps": (MONO | EXPL, 8, 16 * 8 ** 3, 3),
    "pyramid-8-steps": (PYR | EXPL, 8, 16 * 8 ** 3, 3),
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digests_of(name):
    flags, G, n, steps = CASES[name]
    seed = 1000 + sorted(CASES).index(name)
    rng = np.random.default_rng(seed)
    half = G * 2.5
    xyz = rng.uniform(-half * 0.9995, half * 0.9995, (n, 3)).astype(np.float32)
    w = rng.uniform(20.0, 100.0, n).astype(np.float32)
    if steps:
        g = ps.ParticleSystem(ps.default_config(flags=flags, max_particles_num=16384, **GRID[G]))
        assert g.sizes.grid_dim == G
        g.fill_particles(xyz, age=rng.uniform(0.2, 9.0, n).astype(np.float32), w=w,
                         fert_age=rng.uniform(3.0, 12.0, n).astype(np.float32), vxyz=rng.uniform(-8, 8, (n, 3)).astype(np.float32))
        g.step(steps)
        p, counters = g.download_particles(), g.counters
        g.close()
        assert counters["integrated"] > n and counters["births"] > 0
        return {"state": sha(p)}
    g = ps.ParticleSystem(ps.default_config(flags=flags, max_particles_num=16384, collision_radius=1e-6, **GRID[G]))
    assert g.sizes.grid_dim == G
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    age[::17] = 0.5                                      # some kids: exert and feel nothing
    g.fill_particles(xyz, age=age, w=w, fert_age=np.float32(1e6))
    # the probes: half of them on particles (kids among them), half anywhere in the box
    pts = np.zeros((PROBES, 4), np.float32)
    pts[:PROBES // 2, :3] = xyz[:: n // (PROBES // 2)][:PROBES // 2]
    pts[PROBES // 2:, :3] = rng.uniform(-half * 0.9995, half * 0.9995, (PROBES // 2, 3))
    g.init_iframe(); g.build_grid()
    out = g.probe(torch.from_numpy(pts).to(torch.device("cuda", 0)), far=True)
    g.calc_forces_pairs()
    order = np.concatenate([row[1:1 + row[0]] for row in g.download_cellgrid()])
    f = g.download_force4(0, len(order))
    g.calc_forces_apply()
    kills = g.counters["cell_overflow_kills"]
    g.close()
    assert len(order) == n and kills == 0 and out["served"] == PROBES and out["nonfinite"] == 0 and np.abs(f[:, :3]).max() > 0
    assert (f[:, 3].view(np.int32) == 0).all()           # (nobody collided: every adult is on the dense list)
    if name.endswith("ragged"):
        assert int((age >= 1.5).sum()) % 64 != 0
    return {"order": sha(order.astype(np.int32)), "force": sha(f), "probe": sha(out["out4"].cpu().numpy())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library under test was built from (recorded, not checked)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "far_bits.json"))
    a = ap.parse_args()
    res = {"commit": a.commit, "command": "python scripts/far_bits.py --commit " + a.commit, "device": torch.cuda.get_device_name(0),
           "cases": {name: digests_of(name) for name in CASES}}
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
    print(json.dumps(res))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
