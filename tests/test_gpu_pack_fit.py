"""The packs of the force pass's leftovers on the device (plan.hip, k_pack_windows) against the rule (csrc/pack_fit.hpp,
restated in pack_fit_model.py), and the steps that walk them against the oracle, byte for byte.

Packs exist only in the scalar walk of the two-pass stage, which a step takes when the step before it left a hint of at
least 3072 force tasks: 8^3 cells with six full slices each (384 particles and the leftover), collision radius 0 so that
every particle needs a force.  Every case runs one whole step, then the second step by stages: after its pair stage the
launch shape must say scalar walk with pack workgroups, the device's packs must be the model's on the downloaded force
counts, pack for pack, and forces and state must equal the oracle's.  With dt = 0.02 a step moves nobody further than
max_v dt = 0.2, less than the crafted clouds keep from the cells' faces: their per-cell counts hold in the second step
(and a particle of age 3 is neither a kid nor past its life of 300 dt = 6).  The 10^3 grid has 1000 computed cells: 15 windows and one of 40.  The 20^3 grid (8000 cells) is past
what k_plan_force keeps in LDS: the windows' first packs go through global memory there; its forces are compared on
windows of the sorted order, as the full-size tests do."""
import os

import numpy as np
import pytest

import oracle_py as O
import particlesystem_amd as ps
from pack_fit_model import as_rows, best_fit_packs
from util import assert_same_particles, oracle_cfg_from

pytestmark = pytest.mark.gpu
CELL = 5.0


def per_cell_cloud(grid, counts, seed):
    """counts[ix, iy, iz] particles inside every cell, 0.25 away from its faces"""
    rng = np.random.default_rng(seed)
    idx = np.repeat(np.arange(grid ** 3), counts.reshape(-1))
    corner = np.stack(np.unravel_index(idx, (grid,) * 3), 1) * CELL - grid * CELL / 2
    return (corner + rng.uniform(0.25, CELL - 0.25, (len(idx), 3))).astype(np.float32)


def counts_for(case, grid):
    ix = np.indices((grid,) * 3).sum(0)
    if case == "zero":
        return np.full((grid,) * 3, 384)
    if case == "all63":
        return np.full((grid,) * 3, 384 + 63)
    if case == "1and63":
        return np.where(ix & 1, 384 + 63, 384 + 1)
    raise AssertionError(case)


def oracle_pairs(o, lo=0, hi=None):
    o.init_iframe(); o.build_grid()
    total = o.sorted_count()
    f = np.zeros((total + 8, 4), np.float32)
    o.calc_pairs_threads(lo, total if hi is None else hi, f, max(1, min(64, len(os.sched_getaffinity(0)))))
    return f, total


def same_state(g, o, what):
    assert_same_particles(g.download_particles(), o.particles, what)
    qi, q = g.download_queues()
    assert qi.tobytes() == o.queue_info.tobytes() and np.array_equal(q, o.queue), what


def same_forces(g, f, lo, hi):
    got, want = g.download_force4(lo, hi - lo).view(np.uint32), f[lo:hi].view(np.uint32)
    assert np.array_equal(got[:, 3], want[:, 3]), "collision flags differ"
    keep = want[:, 3] == 0                                   # a flagged particle's force is never looked at
    assert np.array_equal(got[keep, :3], want[keep, :3]), "forces differ"


def packs_on_device_are_the_rules(g, leftovers_expected=None):
    packs, shape = g.download_packs()
    assert shape["two_pass"] and not shape["tile"] and shape["pack_workgroups"] > 0, shape      # scalar walk with packs
    r = g.download_force_counts() & 63                       # (one context: the computed cells are all cells, in cell order)
    if leftovers_expected is not None:
        assert set(np.unique(r)) == set(leftovers_expected), np.unique(r)
    want = as_rows(best_fit_packs(r))
    print("packs on the device: %d, cells with a leftover: %d" % (len(packs), int((r > 0).sum())))
    assert len(packs) == len(want)
    assert [tuple(p) for p in packs.tolist()] == want
    return len(packs)


@pytest.mark.parametrize("case, grid, leftovers", [("uniform", 8, None), ("zero", 8, {0}), ("all63", 8, {63}), ("1and63", 8, {1, 63}),
                                                   ("uniform", 10, None)])
def test_second_step_walks_the_rules_packs_and_matches_the_oracle(case, grid, leftovers):
    over = dict(chunk_factor=2, chunk_dim=grid // 2, collision_radius=0.0, dt=0.02)
    n = {8: 215000, 10: 270000}[grid] if case == "uniform" else int(counts_for(case, grid).sum())
    g = ps.ParticleSystem(ps.default_config(max_particles_num=n, **over))
    assert g.sizes.num_cells == grid ** 3 and g.sizes.max_per_cell >= 384 + 63 + 64
    xyz = g.uniform_cloud(n, 77) if case == "uniform" else per_cell_cloud(grid, counts_for(case, grid), 77)
    age, fert = np.float32(3.0), np.float32(1e6)
    o = O.System(oracle_cfg_from(g.cfg))
    assert np.array_equal(g.fill_particles(xyz, age=age, fert_age=fert), o.fill(xyz, age=age, fert_age=fert))
    f, total = oracle_pairs(o)
    o.apply_forces(f)
    g.step(1)
    same_state(g, o, "%s step 1" % case)
    g.init_iframe(); g.build_grid(); g.calc_forces_pairs()
    npacks = packs_on_device_are_the_rules(g, leftovers)
    assert (npacks == 0) == (case == "zero")
    f, total = oracle_pairs(o)
    assert total == n
    same_forces(g, f, 0, total)
    g.calc_forces_apply()
    o.apply_forces(f)
    same_state(g, o, "%s step 2" % case)
    g.close(); o.close()


def test_more_cells_than_the_plan_keeps_in_lds():
    """20^3 = 8000 computed cells (125 windows), ~200 particles each: the windows' first packs go through global memory"""
    n = 1600000
    over = dict(chunk_factor=5, chunk_dim=4, collision_radius=0.0, dt=0.02)
    g = ps.ParticleSystem(ps.default_config(max_particles_num=n, **over))
    assert g.sizes.num_cells == 8000
    xyz = g.uniform_cloud(n, 78)
    o = O.System(oracle_cfg_from(g.cfg))
    assert np.array_equal(g.fill_particles(xyz, age=np.float32(3.0), fert_age=np.float32(1e6)),
                          o.fill(xyz, age=np.float32(3.0), fert_age=np.float32(1e6)))
    g.step(1)
    g.init_iframe(); g.build_grid(); g.calc_forces_pairs()
    packs_on_device_are_the_rules(g)
    # the oracle's particles are the device's after step 1 (the 8^3 and 10^3 cases check step 1; the grids must agree)
    o.particles[:] = g.download_particles()
    o.init_iframe(); o.build_grid()
    assert np.array_equal(g.download_cellgrid(), o.cellgrid)
    total = o.sorted_count()
    f = np.zeros((total + 8, 4), np.float32)
    for lo in (0, total // 2 + 333, total - 4000):
        o.calc_pairs(lo, lo + 4000, f)
        same_forces(g, f, lo, lo + 4000)
    g.calc_forces_apply()
    g.close(); o.close()
