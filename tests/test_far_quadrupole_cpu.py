"""PSAMD_FLAG_FAR_QUADRUPOLE without a GPU (test_far_model_cpu.py has the flag and the entry point): the second moments of hand-made cells; and the METHOD -- the pyramid of monopoles plus the quadrupole term of
every far body (far_model.py, "quadrupole") -- against an fp64 direct sum over all bodies.

The caps (median 2.2e-3, maximum 2.4e-2) are a property of the method, not of the device code: about 2x and 1.4x over the
worst measured, the margins test_far_pyramid_cpu.py uses; and on every cloud the median is at most half the pyramid's.
Measured with that file's clouds and seeds (8192 bodies, 400 sampled), median / maximum relative deviation of |a|, the
pyramid of monopoles -> with quadrupoles: 8^3 cells 2.39e-3 / 4.36e-2 -> 8.35e-4 / 1.38e-2 (uniform) and 1.97e-3 / 1.92e-2 ->
6.82e-4 / 5.08e-3 (clustered); 10^3 cells 5.12e-3 / 3.37e-2 -> 1.06e-3 / 1.17e-2 and 2.41e-3 / 2.62e-2 -> 7.56e-4 / 1.69e-2.  The
medians' ratios: 0.35, 0.35, 0.21, 0.31."""
import numpy as np
import pytest

import far_model as F
from far_harness import hand_made_pyramid, method_against_the_direct_sum


def direct_central(xyz, w):
    """fp64 (X, Y, Z), M and the six central second moments of the bodies about their centre of mass, term by term"""
    x, w = np.asarray(xyz, np.float64), np.asarray(w, np.float64)
    com = (w[:, None] * x).sum(0) / w.sum()
    d = x - com
    return com, w.sum(), np.array([(w * d[:, a] * d[:, b]).sum() for a, b in F.PLANES])


def test_hand_made_cells():
    """6^3 cells, levels 6 and 3 (far_harness.py's hand-made pyramid: every number a short dyadic, so that the float32 planes hold the
    moments exactly).  Two bodies in one cell: C = mu * delta_a * delta_b with the reduced mass mu = 20 * 60 / 80 and delta =
    (1, -1, 0.5); a single body: six exact zeros; a parent of two occupied cells: the moments of its three bodies about their
    centre of mass; repulsion flips all six planes and nothing else"""
    G, cell, xyz, w = hand_made_pyramid()
    lists = F.lists_of(xyz, G)
    assert [len(lists[c]) for c in (cell(0, 0, 0), cell(1, 1, 0), cell(0, 3, 0))] == [2, 1, 1]
    (m0, m1), (c0, c1) = F.level_moments(lists, xyz, w, G, "quadrupole")
    for a, b in zip((m0, m1), F.level_moments(lists, xyz, w, G, "pyramid")[0]):
        assert a.tobytes() == b.tobytes()                             # (X, Y, Z, M are the pyramid's)
    assert c0.dtype == c1.dtype == np.float32 and c0.shape == (216, 6) and c1.shape == (27, 6)
    assert c0[cell(0, 0, 0)].tolist() == [15.0, 15.0, 3.75, -15.0, 7.5, -7.5]
    for c in (cell(1, 1, 0), cell(0, 3, 0)):
        assert c0[c].tobytes() == bytes(24), "a single body has no second moments"
    assert np.count_nonzero(c0.any(1)) == 1
    com, mass, want = direct_central(xyz[:3], w[:3])
    assert m1[0].tolist() == com.tolist() + [mass]
    assert np.abs(c1[0].astype(np.float64) - want).max() <= 1e-9 * np.abs(want).max() and np.abs(want).min() > 1.0
    assert c1[1].tobytes() == bytes(24) and np.count_nonzero(c1.any(1)) == 1      # (the parent of the one body IS that body)
    (r0, r1), (q0, q1) = F.level_moments(lists, xyz, -w, G, "quadrupole")
    for a, b in ((r0, m0), (r1, m1)):
        assert np.array_equal(a[:, :3], b[:, :3]) and np.array_equal(a[:, 3], -b[:, 3])
    for a, b in ((q0, c0), (q1, c1)):
        assert np.array_equal(a, -b) and a.any()                      # (a zero stays +0: x - x is +0 under either sign)


def test_one_adult_per_cell_has_no_second_moments():
    """1000 random bodies, each alone: both products of C_ab round the same real number -- six exact zeros, whatever the bits"""
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-20, 20, (1000, 3)).astype(np.float32)
    w = rng.uniform(20, 100, 1000).astype(np.float32) * rng.choice([-1.0, 1.0], 1000).astype(np.float32)
    s = np.concatenate([F.level_sums([np.array([k])], xyz, w, 1, "quadrupole")[0] for k in range(1000)])
    assert (s[:, 0] != 0).all() and F.central_of(s).tobytes() == bytes(24 * 1000)


@pytest.mark.parametrize("G", [8, 10])
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_the_method_against_the_direct_sum(kind, G):
    quad, mono = method_against_the_direct_sum("quadrupole", kind, G)
    assert np.median(quad) < 2.2e-3
    assert quad.max() < 2.4e-2
    assert np.median(quad) <= 0.5 * np.median(mono)
