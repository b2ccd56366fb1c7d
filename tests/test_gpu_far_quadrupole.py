"""PSAMD_FLAG_FAR_QUADRUPOLE on the device (include/psamd.h, "quadrupoles on the pyramid"): the quadrupole method's cases of the
checks the three far-field methods share (far_force_suite.py has their bodies, docstrings and measured values), and what only
this method has: one adult per cell on one level is the pyramid context byte for byte, the quadrupole part alone, and the gain
in accuracy on the device.

The grids are far_harness.py's (4^3, 6^3, 8^3, 10^3, 16^3 cells)."""
import numpy as np
import pytest

pytest.register_assert_rewrite("far_force_suite")       # (its asserts are this suite's: show their operands)

import far_force_suite as S  # noqa: E402
import far_model as F  # noqa: E402
import particlesystem_amd as ps  # noqa: E402
from far_harness import GRID, box_cloud, frame, low_corner, model_frame  # noqa: E402
from util import assert_same_particles, cloud  # noqa: E402

pytestmark = pytest.mark.gpu

METHOD, PYR, QUAD = "quadrupole", S.PYR, S.QUAD


globals().update(S.tests_of(METHOD))      # the shared checks, this method's cases


# ---- what only this method has ------------------------------------------------------------------------------------------------

def test_one_adult_per_cell_on_one_level_is_the_pyramid_context_byte_for_byte():
    """4^3 cells (one level): an adult in 56 of the 64 cells and 300 kids anywhere -- every C is an exact zero and every
    quadrupole chain +0, so the records of a frame and three whole steps are the PSAMD_FLAG_FAR_PYRAMID context's.  The
    adults start at rest near their cells' centres and three steps move them by little: the last frame's C planes, all
    zeros, show that the condition held to the end"""
    G = 4
    rng = np.random.default_rng(82)
    cells = rng.permutation(G ** 3)[:56]
    corner = np.array([low_corner(c // G % G, c % G, c // (G * G), G) for c in cells])
    adults = (corner + rng.uniform(2.0, 3.0, (56, 3))).astype(np.float32)
    assert sorted(F.cells_of(adults, G).tolist()) == sorted(cells.tolist())
    kids = box_cloud(300, 83, G)
    fill = dict(xyz=np.concatenate([adults, kids]), w=rng.uniform(20.0, 100.0, 356).astype(np.float32), fert_age=np.float32(1e6),
                age=np.concatenate([rng.uniform(15 / 7, 7.5, 56), np.full(300, 0.25)]).astype(np.float32),
                vxyz=np.concatenate([np.zeros((56, 3)), rng.uniform(-8, 8, (300, 3))]).astype(np.float32))
    out = []
    for flags in (QUAD, PYR):
        g = ps.ParticleSystem(ps.default_config(flags=flags, **GRID[G]))
        assert g.sizes.grid_dim == G
        g.fill_particles(**fill)
        g.snapshot_save()
        first = frame(g)
        g.snapshot_restore()
        g.step(3)
        last = frame(g)
        out.append((first, g.download_particles(), g.counters, last))
        g.close()
    (a, pa, ca, la), (b, pb, cb, lb) = out
    assert np.array_equal(a.order, b.order) and np.abs(a.f[:, :3]).max() > 0 and a.f.tobytes() == b.f.tobytes()
    assert a.mom[0].tobytes() == b.mom[0].tobytes() and int((a.mom[0][:, 3] != 0).sum()) == 56
    assert a.cen[0].tobytes() == bytes(24 * G ** 3) and la.cen[0].tobytes() == bytes(24 * G ** 3)
    assert la.f.tobytes() == lb.f.tobytes() and int((la.mom[0][:, 3] != 0).sum()) == 56
    assert_same_particles(pa, pb, "three steps on 4^3 cells, one adult a cell: quadrupoles against the pyramid")
    assert ca == cb and ca["integrated"] >= 3 * 56


def test_the_quadrupole_part_alone():
    """16384 bodies on 8^3 cells: what the flag ADDS -- the record of a quadrupole context minus the record of a pyramid
    context on the same cloud -- against the model's quadrupole part, for the adults whose model part is at least 1e-3 of
    their |a| (78 % of them with this seed; at least a quarter is the condition), relative to |a_q|.  The floor is the fp32
    rounding of two records, a few 2^-23 |a|: about 3e-4 of such an a_q, so 1e-2 leaves some 30x of room, while a wrong
    coefficient or a swapped plane moves a_q by tens of percent.  Measured on an MI355X: 1.4e-4"""
    G, n = 8, 16384
    f, idx, lists, xyz, w_eff, kid = model_frame(G, QUAD, 34, n)
    f0, idx0, _, _, _, _ = model_frame(G, PYR, 34, n)
    assert np.array_equal(idx, idx0) and (f[:, 3].view(np.int32) == 0).all()
    adults = np.nonzero(~kid[idx])[0]
    moments = F.level_moments(lists, xyz, w_eff, G, "quadrupole")
    part = F.quad_accel(lists, xyz, w_eff, G, 0.2, idx[adults], moments)
    whole = F.accel(lists, xyz, w_eff, G, 0.2, idx[adults], "pyramid", (moments[0], None)) + part
    size = np.linalg.norm(part, axis=1)
    use = size >= 1e-3 * np.linalg.norm(whole, axis=1)
    got = f[adults, :3].astype(np.float64) - f0[adults, :3].astype(np.float64)
    rel = np.linalg.norm(got - part, axis=1)[use] / size[use]
    print("quadrupole part alone, %d bodies on %d^3 cells: %.0f %% of the adults qualify, max deviation over |a_q| %.3g"
          % (n, G, 100 * use.mean(), rel.max()))
    assert use.mean() >= 0.25
    assert rel.max() < 1e-2


def test_the_device_is_closer_to_the_direct_sum_with_quadrupoles():
    """8192 bodies on 8^3 cells (test_far_pyramid_cpu.py's uniform cloud, seed 11), 400 sampled, against the fp64 direct sum
    over all bodies: the quadrupole context's median deviation is at most half of the pyramid context's.  Measured on an
    MI355X: median 8.35e-4 against 2.39e-3, a ratio of 0.35 (the maxima: 1.38e-2 against 4.36e-2)"""
    G, n = 8, 8192
    xyz = cloud(n, 11, G * 2.5 * 0.9995)
    pick = np.random.default_rng(13).choice(n, 400, replace=False)
    med = {}
    for flags in (QUAD, PYR):
        f, idx, _, _, w_eff, kid = model_frame(G, flags, 11, n, xyz=xyz, kids=False)
        assert not kid.any()
        got = np.empty((n, 3))
        got[idx] = f[:, :3].astype(np.float64)
        dev = F.rel_dev(got[pick], F.direct(xyz, w_eff, 0.2, pick))
        med[flags] = np.median(dev)
        print("flags %#x, %d bodies on %d^3 cells against the direct sum: median %.3g max %.3g" % (flags, n, G, med[flags], dev.max()))
    assert med[QUAD] <= 0.5 * med[PYR]
