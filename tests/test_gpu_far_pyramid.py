"""PSAMD_FLAG_FAR_PYRAMID on the device (include/psamd.h, "a pyramid of monopoles"): the pyramid's cases of the checks the three
far-field methods share (far_force_suite.py has their bodies, docstrings and measured values), and what only this method has:
on one level (G <= 4) it is the far-monopole context, byte for byte.

The grids are far_harness.py's: 4^3 (one level), 6^3 (levels 6, 3), 8^3 (8, 4), 10^3 (10, 5, 3: an odd level with a ragged parent)
and 16^3 (16, 8, 4)."""
import numpy as np
import pytest

pytest.register_assert_rewrite("far_force_suite")       # (its asserts are this suite's: show their operands)

import far_force_suite as S  # noqa: E402
import particlesystem_amd as ps  # noqa: E402
from far_harness import GRID, frame, lively  # noqa: E402
from util import assert_same_particles  # noqa: E402

pytestmark = pytest.mark.gpu

METHOD, PYR, MONO = "pyramid", S.PYR, S.MONO


globals().update(S.tests_of(METHOD))      # the shared checks, this method's cases


# ---- what only this method has ------------------------------------------------------------------------------------------------

def test_one_level_is_the_far_monopole_context_byte_for_byte():
    """G = 4: one level, one block of 64 cells -- the records of a frame and three whole steps (births on) are those of a
    PSAMD_FLAG_FAR_MONOPOLE context given the same fill: its 15 empty parts add +0"""
    c = lively(2048, 81, 4)
    out = []
    for flag in (PYR, MONO):
        g = ps.ParticleSystem(ps.default_config(flags=flag | ps.FLAG_EXPLOSIONS, **GRID[4]))
        assert g.sizes.grid_dim == 4
        g.fill_particles(**c)
        g.snapshot_save()
        fr = frame(g)
        g.snapshot_restore()
        g.step(3)
        out.append((fr.order, fr.f, g.download_particles(), g.counters))
        g.close()
    (oa, fa, pa, ca), (ob, fb, pb, cb) = out
    assert np.array_equal(oa, ob) and np.abs(fa[:, :3]).max() > 0 and fa.tobytes() == fb.tobytes()
    assert_same_particles(pa, pb, "three steps on 4^3 cells, pyramid against far monopoles")
    assert ca == cb and ca["integrated"] > 3000 and ca["births"] > 0
