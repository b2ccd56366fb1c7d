"""SHA-256 digests of what far_bits.py does not pin: quadrupole contexts (PSAMD_FLAG_FAR_QUADRUPOLE: force records and far
probes with their quadrupole terms, acceleration and potential together and each alone), psamd_potential in every form
(cutoff, lists longer than one chain, all-pairs, flat, pyramid, quadrupoles), probes outside the far field (all-pairs, cutoff
exact and fast, the generic exact arithmetic of a softening outside the lean range) and three whole steps with explosions on
a quadrupole context.

    python scripts/field_bits.py --commit <the commit the library was built from> [--out tests/golden/field_bits.json]

The shape is far_bits.py's, and so is the use: only the public Python API, so the same file runs on any commit that has the
quadrupole flag; the committed tests/golden/field_bits.json was written on one MI355X at the commit it names;
tests/test_gpu_field_bits.py recomputes the digests with digests_of() and compares.  The cases have a table and a seed rule
of their own (a case's seed is a checksum of its name), so that neither table moves the other's frames.  A digest that differs
means that a refactor of the field walks changed an association: the code is wrong then, not the file."""
import argparse
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: one HIP runtime)

import particlesystem_amd as ps  # noqa: E402
from far_bits import GRID, PROBES, sha  # noqa: E402

MONO, PYR, FAST, EXPL, ALLP = ps.FLAG_FAR_MONOPOLE, ps.FLAG_FAR_PYRAMID, ps.FLAG_FAST_MATH, ps.FLAG_EXPLOSIONS, ps.FLAG_ALL_PAIRS
QUAD = ps.FLAG_FAR_PYRAMID | ps.FLAG_FAR_QUADRUPOLE
LONG = dict(chunk_factor=2, chunk_dim=3, x_factor=4)     # 6^3 cells with room for lists of 304: 60 a cell in the mean fit
GENERIC = dict(eps2=1e-8)                                # eps2^3 below 2^-60: outside the lean range, the generic exact forms

# name: (what, flags, G, bodies, configuration beside GRID[G])
#   "force"      the sorted order, the force records, 256 probes of acceleration and potential (far contexts: the far form)
#   "fields"     ... and the probes of the acceleration alone and of the potential alone (other instances of the kernel)
#   "potential"  psamd_potential: phi in export order and the result record; two bodies at one point
#   "probe"      the 256 probes alone
#   "steps"      the exported state after three whole steps
CASES = {
    "quad-10-exact": ("force", QUAD, 10, 16 * 10 ** 3, {}),           # levels 10, 5, 3: odd sizes, clamped boxes
    "quad-10-fast": ("force", QUAD | FAST, 10, 16 * 10 ** 3, {}),
    "quad-16-exact": ("force", QUAD, 16, 4 * 16 ** 3, {}),            # a wave's 64 particles span many cells and several parents
    "quad-8-ragged": ("fields", QUAD, 8, 5003, {}),                   # the last dense task is not full
    "potential-cutoff-8": ("potential", 0, 8, 16 * 8 ** 3, {}),
    "potential-cutoff-6-long": ("potential", 0, 6, 60 * 6 ** 3, LONG),      # lists longer than POT_CHAIN (64) in some cells
    "potential-allpairs-6": ("potential", ALLP, 6, 16 * 6 ** 3, {}),  # 216 cells: four blocks, the last one padded
    "potential-flat-6": ("potential", MONO, 6, 16 * 6 ** 3, {}),
    "potential-pyramid-10": ("potential", PYR, 10, 16 * 10 ** 3, {}),
    "potential-quad-10": ("potential", QUAD, 10, 16 * 10 ** 3, {}),
    "probe-allpairs-6": ("probe", ALLP, 6, 16 * 6 ** 3, {}),
    "probe-cutoff-8-exact": ("probe", 0, 8, 16 * 8 ** 3, {}),
    "probe-cutoff-8-fast": ("probe", FAST, 8, 16 * 8 ** 3, {}),
    "probe-cutoff-8-generic": ("probe", 0, 8, 16 * 8 ** 3, GENERIC),
    "quad-8-steps": ("steps", QUAD | EXPL, 8, 16 * 8 ** 3, {}),
}


def digests_of(name):
    what, flags, G, n, over = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    half = G * 2.5
    xyz = rng.uniform(-half * 0.9995, half * 0.9995, (n, 3)).astype(np.float32)
    w = rng.uniform(20.0, 100.0, n).astype(np.float32)
    cfg = dict(GRID[G], flags=flags, max_particles_num=16384)
    cfg.update(over)
    if what == "steps":
        g = ps.ParticleSystem(ps.default_config(**cfg))
        assert g.sizes.grid_dim == G
        g.fill_particles(xyz, age=rng.uniform(0.2, 9.0, n).astype(np.float32), w=w,
                         fert_age=rng.uniform(3.0, 12.0, n).astype(np.float32), vxyz=rng.uniform(-8, 8, (n, 3)).astype(np.float32))
        g.step(3)
        p, counters = g.download_particles(), g.counters
        g.close()
        assert counters["integrated"] > n and counters["births"] > 0
        return {"state": sha(p)}
    far = dict(far=True, quadrupole=bool(flags & ps.FLAG_FAR_QUADRUPOLE)) if flags & (MONO | PYR) else {}
    g = ps.ParticleSystem(ps.default_config(collision_radius=1e-6, **cfg))
    assert g.sizes.grid_dim == G
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    age[::17] = 0.5                                      # some kids: exert and feel nothing
    if what == "potential":
        xyz[2] = xyz[1]                                  # two adults at one point: they see each other
    g.fill_particles(xyz, age=age, w=w, fert_age=np.float32(1e6))
    # the probes: half of them on particles (kids among them), half anywhere in the box
    pts = np.zeros((PROBES, 4), np.float32)
    pts[:PROBES // 2, :3] = xyz[:: n // (PROBES // 2)][:PROBES // 2]
    pts[PROBES // 2:, :3] = rng.uniform(-half * 0.9995, half * 0.9995, (PROBES // 2, 3))
    pts = torch.from_numpy(pts).to(torch.device("cuda", 0))
    g.init_iframe(); g.build_grid()
    res = {}
    if what == "potential":
        out = g.potential(phi=True, **far)
        counts = np.concatenate([row[:1] for row in g.download_cellgrid()])
        assert out["listed"] > 0 and out["nonfinite"] == 0 and len(out["phi"]) == n
        if name.endswith("long"):
            assert counts.max() > 64
        res["phi"] = sha(out["phi"].cpu().numpy())
        res["record"] = sha(np.array([out["listed"], out["nonfinite"]], np.int64)) + sha(np.array([out["potential"], out["phi_min"], out["phi_max"]], np.float64))
    else:
        probes = {"probe": dict(acc=True, phi=True)}
        if what == "fields":
            probes.update({"probe_acc": dict(acc=True, phi=False), "probe_phi": dict(acc=False, phi=True)})
        for key, fields in probes.items():
            out = g.probe(pts, **fields, **far)
            assert out["served"] == PROBES and out["nonfinite"] == 0
            res[key] = sha(out["out4"].cpu().numpy())
    if what in ("force", "fields"):
        g.calc_forces_pairs()
        order = np.concatenate([row[1:1 + row[0]] for row in g.download_cellgrid()])
        f = g.download_force4(0, len(order))
        g.calc_forces_apply()
        assert len(order) == n and np.abs(f[:, :3]).max() > 0
        assert (f[:, 3].view(np.int32) == 0).all()       # (nobody collided: every adult is on the dense list)
        if name.endswith("ragged"):
            assert int((age >= 1.5).sum()) % 64 != 0
        res.update({"order": sha(order.astype(np.int32)), "force": sha(f)})
    kills = g.counters["cell_overflow_kills"]
    g.close()
    assert kills == 0
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library under test was built from (recorded, not checked)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "field_bits.json"))
    a = ap.parse_args()
    res = {"commit": a.commit, "command": "python scripts/field_bits.py --commit " + a.commit, "device": torch.cuda.get_device_name(0),
           "cases": {name: digests_of(name) for name in CASES}}
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
    print(json.dumps(res))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
