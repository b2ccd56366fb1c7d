"""PSAMD_FLAG_FAR_MONOPOLE on the device (include/psamd.h, "long-range gravity"): the flat method's cases of the checks the three
far-field methods share (far_force_suite.py has their bodies, docstrings and measured values, and tests_of() makes the cases), and what only this method has:
one adult per cell is the all-pairs force, and once one size up against an fp64 direct sum.

The small contexts use 8^3 cells of about 16 bodies (far_harness.py's GRID) unless noted."""
import numpy as np
import pytest

pytest.register_assert_rewrite("far_force_suite")       # (its asserts are this suite's: show their operands)

import far_force_suite as S  # noqa: E402
import far_model as F  # noqa: E402
import particlesystem_amd as ps  # noqa: E402
from far_harness import frame, index_of  # noqa: E402
from util import cloud  # noqa: E402

pytestmark = pytest.mark.gpu

METHOD, MONO, REL = "flat", S.MONO, S.REL


globals().update(S.tests_of(METHOD))      # the shared checks, this method's cases


# ---- what only this method has ------------------------------------------------------------------------------------------------

def test_one_adult_per_cell_is_the_direct_sum():
    """no cell holds two: every monopole IS its cell's particle, the result is the all-pairs force up to association"""
    G = 16
    xyz = cloud(5000, 44, 39.98)
    _, first = np.unique(F.cells_of(xyz, G), return_index=True)
    xyz = xyz[np.sort(first)]
    n = len(xyz)
    assert 2500 < n < 3500
    g = ps.ParticleSystem(ps.default_config(flags=MONO, collision_radius=1e-6))
    ids = g.fill_particles(xyz, age=np.float32(3.0), fert_age=np.float32(1e6))
    fr = frame(g)
    idx = index_of(g, ids)[fr.order]
    occupied = np.nonzero(fr.mom[0][:, 3] != 0)[0]
    assert len(occupied) == n and max(len(l) for l in fr.lists) == 1
    assert np.array_equal(fr.mom[0][F.cells_of(xyz, G)], np.concatenate([xyz, np.full((n, 1), 60.0, np.float32)], 1))
    want = F.direct(xyz, np.full(n, 60.0, np.float32), 0.2, idx)
    rel = F.rel_dev(fr.f[:, :3].astype(np.float64), want)
    print("one adult per cell, %d bodies on 16^3 cells: max relative deviation from the fp64 direct sum %.3g" % (n, rel.max()))
    assert (fr.f[:, 3].view(np.int32) == 0).all() and rel.max() < REL
    g.close()


def test_n_2_18_against_the_direct_sum_and_the_cutoff_steps_counters():
    """N = 2^18 on the default grid (64 to a cell): 200 served particles against an fp64 direct sum over all 2^18 bodies, the
    caps of the method (test_far_monopole_cpu.py); collisions are untouched, so the step's counters are the cutoff context's"""
    n = 1 << 18
    g = ps.ParticleSystem(ps.default_config(flags=MONO))
    b = ps.ParticleSystem(ps.default_config())
    xyz = g.uniform_cloud(n, 18)
    rng = np.random.default_rng(18)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    for s in (g, b):
        ids = s.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    fr = frame(g)
    b.step(1)
    cg, cb = g.counters, b.counters
    assert cg["integrated"] == cb["integrated"] > n // 2 and cg["deaths_collision"] == cb["deaths_collision"] > 0
    idx = index_of(g, ids)[fr.order]
    served = np.nonzero(fr.f[:, 3].view(np.int32) == 0)[0]
    pick = rng.choice(served, 200, replace=False)
    want = F.direct(xyz, np.full(n, 60.0, np.float32), 0.2, idx[pick], chunk=25)
    rel = F.rel_dev(fr.f[pick, :3].astype(np.float64), want)
    print("far monopoles at N=2^18 vs fp64 direct sum (200 particles): median %.3g max %.3g" % (np.median(rel), rel.max()))
    assert rel.max() < 5e-2 and np.median(rel) < 5e-3
    g.close(); b.close()
