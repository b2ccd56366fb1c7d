"""PSAMD_FLAG_FAR_PYRAMID without a GPU (test_far_model_cpu.py has the flag and the entry points): psamd_far_levels; the partition property of the far set; and the METHOD -- the stencil as a direct sum,
coarser monopoles for farther mass (far_model.py, "pyramid") -- against an fp64 direct sum over all bodies.

The caps (median 1e-2, maximum 6e-2, the stencil alone above 0.5) are a property of the method, not of the device code: about
2x and 1.4x over the worst measured, the margins test_far_monopole_cpu.py uses.  Measured with the seeds below, 8192 bodies, 400
sampled per cloud, median / maximum relative deviation of |a|: 8^3 cells 2.4e-3 / 4.4e-2 (uniform) and 2.0e-3 / 1.9e-2
(clustered); 10^3 cells (levels 10, 5, 3: an odd level with a ragged parent) 5.1e-3 / 3.4e-2 and 2.4e-3 / 2.6e-2; the stencil
alone: median 0.77 to 0.92."""
import ctypes

import numpy as np
import pytest

import far_model as F
import particlesystem_amd as ps
from far_harness import hand_made_pyramid, method_against_the_direct_sum


@pytest.mark.parametrize("factor,dim,want", [(1, 4, [4]), (2, 3, [6, 3]), (2, 4, [8, 4]), (2, 5, [10, 5, 3]), (4, 4, [16, 8, 4]),
                                             (8, 5, [40, 20, 10, 5, 3])])
def test_far_levels(factor, dim, want):
    cfg = ps.default_config(chunk_factor=factor, chunk_dim=dim)
    assert ps.describe(cfg)[0].grid_dim == want[0]
    assert ps.far_levels(cfg) == want == F.levels_of(want[0])
    n, dims = ctypes.c_int32(), (ctypes.c_int32 * 16)(*([-1] * 16))
    assert ps.load().psamd_far_levels(ctypes.byref(cfg), ctypes.byref(n), dims) == 0
    assert n.value == len(want) and list(dims) == want + [0] * (16 - len(want))


def cells_to_cover(G):
    """every cell up to 16^3.  Of the deep grids (far_harness.DEEP's 20^3 and 36^3, where the model is the device's reference) every
    cell with a coordinate among 0, 1, G - 2, G - 1 or under the one child of a ragged parent, and 500 more by a seeded choice"""
    if G <= 16:
        return range(G ** 3)
    dims = F.levels_of(G)
    edge = {0, 1, G - 2, G - 1}
    for lvl in range(1, len(dims) - 1):
        if dims[lvl] % 2:                                               # the level's last cell is the next level's last parent's one child
            edge.update(range((dims[lvl] - 1) << lvl, G))
    i1, i2, i3 = np.unravel_index(np.arange(G ** 3), (G, G, G))
    at = np.isin(i1, list(edge)) | np.isin(i2, list(edge)) | np.isin(i3, list(edge))
    at[np.random.default_rng(17).choice(G ** 3, 500, replace=False)] = True
    return np.nonzero(at)[0]


@pytest.mark.parametrize("G", [4, 6, 8, 10, 16, 20, 36])
def test_stencil_and_set_cover_every_cell_exactly_once(G):
    sizes, cells = [], cells_to_cover(G)
    for c in cells:
        members = F.far_set(c, G, "pyramid")
        n = F.coverage(c, G, "pyramid", members)
        assert (n == 1).all(), "cell %d of %d^3: %d cells not covered once" % (c, G, (n != 1).sum())
        sizes.append(len(members))
    print("%d^3 cells, %d of them: %.0f far bodies a particle in the mean (flat: %.0f)"
          % (G, len(cells), np.mean(sizes), np.mean([G ** 3 - len(F.stencil_cells(c, G)) for c in cells])))


@pytest.mark.parametrize("G", [8, 10])
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_the_method_against_the_direct_sum(kind, G):
    far, near = method_against_the_direct_sum("pyramid", kind, G)
    assert np.median(far) < 1e-2
    assert far.max() < 6e-2
    assert np.median(near) > 0.5


def test_a_hand_made_pyramid():
    """6^3 cells, levels 6 and 3.  Two occupied cells under one parent: the parent is their joint centre of mass, the sums
    taken in child order; one occupied cell under another parent: the parent IS that cell; the cells' own moments are the
    flat method's; repulsion flips M alone, at every level"""
    G, cell, xyz, w = hand_made_pyramid()
    assert F.cells_of(xyz, G).tolist() == [cell(0, 0, 0), cell(0, 0, 0), cell(1, 1, 0), cell(0, 3, 0)]
    lists = F.lists_of(xyz, G)
    m0, m1 = F.level_moments(lists, xyz, w, G, "pyramid")[0]
    assert np.array_equal(m0, F.level_moments(lists, xyz, w, G, "flat")[0][0])
    assert m0[cell(0, 0, 0)].tolist() == [-13.25, 13.25, 14.375, 80.0]
    assert m1[0].tolist() == [np.float32((20.0 * -14.0 + 60.0 * -13.0 + 80.0 * -8.0) / 160.0), 11.125, 13.1875, 160.0]
    assert m1[1].tolist() == [1.0, 14.0, 14.0, 40.0] == m0[cell(0, 3, 0)].tolist()
    assert (m1[:, 3] != 0).sum() == 2 and (m0[:, 3] != 0).sum() == 3
    r0, r1 = F.level_moments(lists, xyz, -w, G, "pyramid")[0]
    for a, b in ((r0, m0), (r1, m1)):
        assert np.array_equal(a[:, :3], b[:, :3]) and np.array_equal(a[:, 3], -b[:, 3])
