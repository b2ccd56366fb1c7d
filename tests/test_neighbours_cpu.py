"""The numpy model of psamd_neighbours (tests/neighbours_model.py) against an fp64 brute force over the same stencil, its own
invariants, and the header's declarations.  No GPU: the frames are the oracle's (fill, init_iframe, build_grid), whose particle
records and cell grid are what a context downloads.

Exactness.  On a lattice cloud every coordinate is a multiple of 2^-6 inside +-20 and the radius is a multiple of 2^-6: a
difference is a multiple of 2^-6 below 2^6 (12 bits), its square a multiple of 2^-12 below 2^12 (24 bits), and the sums stay
multiples of 2^-12 below 2^14 -- but only 24 bits are kept, so the sums are exact where they are below 2^12.  The test is
d2 <= r2 with r2 <= 25: a sum that reaches 2^12 is far beyond it whichever way it was rounded, and every sum below 2^12 is
exact.  The model's sets therefore equal the fp64 sets with no pair left out.

On a uniform random cloud the fp32 d2 differs from the exact one by a few 2^-24 relative, so the sets can differ only for
pairs whose fp64 distance lies within a relative 1e-5 of the radius (fifty times the rounding); the share of within-radius
pairs in that shell is about 3 * 1e-5 * 2 = 6e-5 by its volume, and the test asks that it stays under 1e-3 -- a condition on
the cloud, not a tolerance on the model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import neighbours_model as M
import oracle_py as O
import particlesystem_amd as ps

SMALL = dict(chunk_factor=2, chunk_dim=4)          # an 8^3 grid of 5-unit cells: the box is [-20, 20)^3
KID, ADULT = np.float32(0.5), np.float32(3.0)


def frame(xyz, age, **over):
    o = O.System(O.default_config(**{**SMALL, **over}))
    ids = o.fill(xyz, age=age, fert_age=np.float32(1e6))
    o.init_iframe()
    o.build_grid()
    assert 0.5 < o.d.kid_age < 3.0
    fr = M.Frame(o.particles.copy(), o.cellgrid.copy(), o.d.grid_dim, o.d.kid_age, o.d.max_per_cell)
    fr.filled = ids.astype(np.int64)          # the slot every input row went to
    o.close()
    return fr


def lattice_cloud(n, seed, half=20.0, centre=0.0):
    rng = np.random.default_rng(seed)
    return (centre + rng.integers(int(-half * 64) + 1, int(half * 64), (n, 3)) / 64.0).astype(np.float32)


def ages(n, seed, kids=7):
    a = np.full(n, ADULT, np.float32)
    a[np.random.default_rng(seed).integers(0, kids, n) == 0] = KID
    return a


@pytest.mark.parametrize("radius", [5.0, 1.0, 0.390625, 2.5])
def test_lattice_clouds_equal_the_fp64_brute_force(radius):
    xyz = np.concatenate([lattice_cloud(3000, 1), lattice_cloud(600, 2, 3.0, 10.0)])       # a dense blob inside a chunk: many pairs at the small radii
    fr = frame(xyz, ages(len(xyz), 3), max_particles_num=1 << 18)
    assert radius * 64 == int(radius * 64)
    got = M.neighbours(fr, radius)
    want, _, _, _ = M.brute_sets(fr, radius)
    assert got["listed"] == len(want) == len(xyz)
    pairs = 0
    for i, s in want.items():
        mine = got["lists"][i]
        assert len(set(mine.tolist())) == len(mine) and set(mine.tolist()) == s, (radius, i)
        pairs += len(s)
    assert got["pairs"] == pairs > 0


def test_uniform_random_cloud_agrees_outside_a_thin_shell():
    radius, n = 1.0, 4096
    rng = np.random.default_rng(11)
    xyz = rng.uniform(4.0, 16.0, (n, 3)).astype(np.float32)          # 4096 bodies in a few cells of one chunk: thousands of pairs within 1.0
    fr = frame(xyz, ages(n, 12), max_particles_num=1 << 18)
    got = M.neighbours(fr, radius)
    want, q, c, dist = M.brute_sets(fr, radius)
    assert got["listed"] == n
    near = np.abs(dist - radius) <= 1e-5 * radius
    shell = set(zip(q[near].tolist(), c[near].tolist()))
    within = int((dist <= radius).sum())
    share = len([1 for k in np.nonzero(near)[0] if dist[k] <= radius]) / within
    print("uniform cloud: %d pairs within the radius, %d in the shell, share of within-radius pairs left to the shell %.3g" % (within, len(shell), share))
    assert within > 10000 and share <= 1e-3
    for i, s in want.items():
        mine = set(got["lists"][i].tolist())
        assert all((i, j) in shell for j in mine ^ s), (i, mine ^ s)


def mixed_frame():
    xyz = np.concatenate([lattice_cloud(2500, 21, 9.0, 10.0),
                          [(11.0, 11.0, 11.0), (11.0, 11.0, 11.0)],            # two at one point
                          [(11.5, 11.0, 11.0)]]).astype(np.float32)             # a kid beside them
    age = ages(len(xyz), 22)
    age[-3:] = (ADULT, ADULT, KID)
    return frame(xyz, age, max_particles_num=1 << 18), len(xyz)


def test_symmetry_kids_and_coincident_particles():
    fr, n = mixed_frame()
    got = M.neighbours(fr, 2.0)
    lists, kid = got["lists"], fr.kid
    kids = [i for i in lists if kid[i]]
    assert len(kids) > 100
    for i, mine in lists.items():
        assert not kid[mine].any(), "a kid is somebody's neighbour"
        if not kid[i]:
            for j in mine:                      # two adults inside their lists list each other
                assert i in lists[int(j)], (i, j)
    assert any(len(lists[i]) > 0 for i in kids), "no kid has a neighbour"
    a, b, k = (int(i) for i in fr.filled[-3:])
    assert b in lists[a] and a in lists[b] and got["d2_min"] == 0.0
    assert a in lists[k] and b in lists[k] and k not in lists[a] and k not in lists[b]
    # nearest: the smallest d2, ties to the lower id (a and b are equally far from the kid)
    at = {int(i): p for p, i in enumerate(got["ids"])}
    assert got["nearest"][at[k]] == min(a, b) and got["nearest_d2"][at[k]] == np.float32(0.25)
    assert got["nearest"][at[a]] == b and got["nearest"][at[b]] == a


def test_csr_consistency_and_the_names():
    fr, n = mixed_frame()
    fr.live = np.concatenate([fr.live, [len(fr.xyz)]])          # one more live slot that is in no list of the frame
    fr.xyz = np.concatenate([fr.xyz, [[0.0, 0.0, 0.0]]]).astype(np.float32)
    fr.kid = np.concatenate([fr.kid, [False]])
    got = M.neighbours(fr, 2.0)
    assert got["count"][-1] == -1 and got["nearest"][-1] == -1 and np.isposinf(got["nearest_d2"][-1])
    assert np.array_equal(np.diff(got["offsets"]), np.maximum(got["count"], 0)) and got["offsets"][0] == 0
    assert got["offsets"][-1] == got["wanted"] == len(got["list"]) == got["pairs"]
    assert got["max_count"] == got["count"].max() and got["listed"] == n
    for p, i in enumerate(got["ids"][:-1]):
        assert np.array_equal(got["list"][got["offsets"][p]:got["offsets"][p + 1]], got["lists"][int(i)])
    # a capacity cuts the arrays, not the record's counts
    short = M.neighbours(fr, 2.0, capacity=100)
    assert len(short["count"]) == 100 and short["wanted"] == got["offsets"][100] and short["pairs"] == got["pairs"]
    assert np.array_equal(short["list"], got["list"][:short["wanted"]])
    # by index: the same lists through the export order
    by = M.neighbours(fr, 2.0, index=True)
    assert np.array_equal(got["ids"][by["list"]], got["list"]) and np.array_equal(by["offsets"], got["offsets"])
    has = by["nearest"] >= 0
    assert np.array_equal(got["ids"][by["nearest"][has]], got["nearest"][has]) and np.array_equal(has, got["nearest"] >= 0)


def test_the_header_and_the_python_mirror_agree():
    """fails without the service: the header declares the functions and both struct sizes, the mirror's sizes agree, the
    library exports the symbols"""
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "psamd.h")).read()
    assert re.search(r"\bint psamd_neighbours\(psamd_ctx \*ctx, const psamd_neighbours_spec \*spec\);", text)
    assert re.search(r"\bint psamd_neighbours_result_get\(psamd_ctx \*ctx, psamd_neighbours_result \*out\);", text)
    assert re.search(r"\}\s*psamd_neighbours_spec;\s*/\* 72 bytes \*/", text) and re.search(r"\}\s*psamd_neighbours_result;\s*/\* 40 bytes \*/", text)
    assert "#define PSAMD_ABI_VERSION 8" in text and ps.ABI_VERSION == 8
    assert C.sizeof(ps.NeighboursSpec) == 72 and C.sizeof(ps.NeighboursResult) == 40
    assert ps.NeighboursSpec.capacity.offset == 40 and ps.NeighboursSpec.result_dev.offset == 64 and ps.NeighboursResult.d2_min.offset == 32
    names = {row[0] for row in ps.ABI}
    assert {"psamd_neighbours", "psamd_neighbours_result_get", "psamd_download_neighbours"} <= names
    lib = ps.load()
    assert lib.psamd_abi_version() == 8 and all(hasattr(lib, n) for n in names)
