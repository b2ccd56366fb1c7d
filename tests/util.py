"""Shared helpers for the parity tests (oracle side is test infrastructure)."""
import os

import numpy as np

import oracle_py as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M64 = (1 << 64) - 1


def g2_cloud():
    return np.fromfile(os.path.join(GOLDEN, "g2_cloud_n4096_seed12345.f32"), dtype=np.float32).reshape(-1, 3)


def cloud(n, seed, half=40.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-half, half, (n, 3)).astype(np.float32)


def oracle_cfg_from(cfg):
    """psamd Config -> oracle Config (same reference constants)."""
    return O.default_config(**{k: getattr(cfg, k) for k in
                               ("max_particles_num", "x_factor", "chunk_factor", "chunk_dim", "cell_size",
                                "eps2", "collision_radius", "particle_weight", "dt", "max_v",
                                "explosion_speed", "life_steps")})


def oracle_from(cfg):
    """an oracle system with the reference constants AND the options of a psamd Config"""
    o = O.System(oracle_cfg_from(cfg))
    o.set_options(**O.options_from(cfg))
    return o


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def explosion_rng(seed):
    """The product's counter-based explosion RNG restated for the oracle's callback
    (apply.hip k_apply / lifecycle.hip commit_move): keyed on (seed, step, parent id)."""
    def fn(pid, step):
        h0 = splitmix64(seed ^ ((step & 0xFFFFFFFF) << 32) ^ (pid & 0xFFFFFFFF))
        h1 = splitmix64(h0)
        h2 = splitmix64(h1)
        h3 = splitmix64(h2)
        ints = tuple(int((h >> 11) * (1.0 / 9007199254740992.0) * 100.0) - 50 for h in (h0, h1, h2))
        return ints, (h3 >> 11) * (1.0 / 9007199254740992.0)
    return fn


def assert_same_particles(gpu_p, ora_p, what=""):
    """Bit-exact comparison of two P_DATA_TYPE arrays, with a readable diff."""
    if gpu_p.tobytes() == ora_p.tobytes():
        return
    for f in gpu_p.dtype.names:
        a, b = gpu_p[f], ora_p[f]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.nonzero(a != b)[0]
        if len(bad):
            k = bad[0]
            raise AssertionError("%s field %s differs at %d slots, first slot %d: gpu %r oracle %r" %
                                 (what, f, len(bad), k, gpu_p[f][k], ora_p[f][k]))
    ga = np.frombuffer(gpu_p.tobytes(), np.uint8).reshape(-1, 72)
    oa = np.frombuffer(ora_p.tobytes(), np.uint8).reshape(-1, 72)
    rows, cols = np.nonzero(ga != oa)
    raise AssertionError("%s records differ only in padding bytes: %d slots, first slot %d byte %d gpu %d oracle %d, cell there %d" %
                         (what, len(set(rows.tolist())), rows[0], cols[0], ga[rows[0], cols[0]], oa[rows[0], cols[0]], gpu_p["cell"][rows[0]]))


# ---- a container that is no whole number of slot tiles (the GPU tests of export, potential and remove) ----------------------
SLOT_TILE = 4096          # the slot walk's tile (slot_walk.hpp)
RAGGED = dict(chunk_factor=2, chunk_dim=4, max_particles_num=4096)
CAPACITIES = (0, 1, 63, 64, 65, -1, 0, +1)          # the last three: relative to the live count
SENTINEL = -0x12345679


def ragged(seed=31, **over):
    """(context, its live records): uniform_cloud(4096, seed) in 125 segments of 144 slots = 18 000 slots, four tiles and
    one of 1616, with a live particle in the partial tile"""
    import particlesystem_amd as ps
    g = ps.ParticleSystem(ps.default_config(**RAGGED, **over))
    rng = np.random.default_rng(seed)
    g.fill_particles(g.uniform_cloud(4096, seed), age=rng.uniform(0.2, 9.0, 4096).astype(np.float32), fert_age=np.float32(1e6),
                     w=rng.uniform(20.0, 100.0, 4096).astype(np.float32), vxyz=rng.uniform(-20, 20, (4096, 3)).astype(np.float32))
    slots = g.owned_slots()
    assert slots % SLOT_TILE != 0 and slots > SLOT_TILE, slots
    p = g.download_particles()
    rec = p[(p["cell"] >= 0) & (p["cell"] < g.sizes.num_cells)]
    assert rec["id"].max() >= max(8192, slots // SLOT_TILE * SLOT_TILE), (rec["id"].max(), slots)
    return g, rec


def capacities(live):
    return [c if k < 5 else live + c for k, c in enumerate(CAPACITIES)]
