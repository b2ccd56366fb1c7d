"""The numpy model of psamd_groups (tests/groups_model.py) against an independent brute force, its own invariants, the shapes
of the clouds test_gpu_groups.py runs, and the header's declarations.  No GPU: the frames are the oracle's (fill, init_iframe,
build_grid), whose particle records and cell grid are what a context downloads.

The brute force shares the model's fp32 d2 (neighbours_model.d2_fp32: the arithmetic is the definition) and nothing else: a
dense boolean adjacency over all members at once, cut to the pairs of cells that are in each other's stencil, closed by
repeated breadth-first search."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import groups_model as GM
import neighbours_model as M
import oracle_py as O
import particlesystem_amd as ps
from test_gpu_neighbours import CS, GRIDS, SPECIAL

ADULT = np.float32(3.0)


def frame(xyz, age, G=4, **over):
    o = O.System(O.default_config(**{**GRIDS[G], **over}))
    ids = o.fill(xyz, age=age, fert_age=np.float32(1e6))
    o.init_iframe()
    o.build_grid()
    assert o.d.grid_dim == G and 0.5 < o.d.kid_age < 3.0
    fr = M.Frame(o.particles.copy(), o.cellgrid.copy(), o.d.grid_dim, o.d.kid_age, o.d.max_per_cell)
    fr.filled = ids.astype(np.int64)          # the slot every input row went to
    fr.cap = int(o.d.max_per_cell)
    o.close()
    return fr


def adults(xyz):
    return np.full(len(xyz), ADULT, np.float32)


@functools.lru_cache(maxsize=None)
def rough(G, kids=True):
    o = O.System(O.default_config(**GRIDS[G]))
    cap = int(o.d.max_per_cell)
    o.close()
    xyz, age = GM.rough_groups_cloud(G, cap)
    fr = frame(xyz, age if kids else adults(xyz), G)
    assert fr.cap == cap
    return fr


@functools.lru_cache(maxsize=None)
def snake_frame(gap_at=None):
    xyz, chain = GM.snake(gap_at)
    fr = frame(xyz, adults(xyz))
    fr.chain = fr.filled[chain]               # the chain's k-th point's slot
    return fr


@functools.lru_cache(maxsize=None)
def near_miss_frame():
    xyz, radius = GM.near_miss()
    return frame(xyz, adults(xyz)), radius


@functools.lru_cache(maxsize=None)
def clump_frame():
    xyz = GM.clump()
    return frame(xyz, adults(xyz), max_particles_num=16384)


def brute_roots(fr, radius):
    """per slot the smallest slot of its component (-1: no member), by the dense adjacency and breadth-first search"""
    n = len(fr.xyz)
    cell = np.full(n, -1, np.int64)
    for c in fr.cells():
        cell[fr.lists[c]] = c
    mem = np.nonzero((cell >= 0) & ~fr.kid)[0]
    near = np.zeros((fr.num_cells, fr.num_cells), bool)
    for c in range(fr.num_cells):
        near[c, list(M.stencil(c, fr.G))] = True
    r2 = np.float32(np.float32(radius) * np.float32(radius))
    with np.errstate(invalid="ignore", over="ignore"):
        adj = (M.d2_fp32(fr.xyz[mem], fr.xyz[mem]) <= r2) & near[cell[mem]][:, cell[mem]]
    np.fill_diagonal(adj, False)
    assert np.array_equal(adj, adj.T), "the relation is not symmetric"
    comp = np.full(len(mem), -1, np.int64)
    for s in range(len(mem)):                 # ascending slot id: the start of a search is its component's smallest member
        if comp[s] >= 0:
            continue
        comp[s] = s
        front = np.array([s])
        while len(front):
            reach = adj[front].any(0) & (comp < 0)
            comp[reach] = s
            front = np.nonzero(reach)[0]
    root = np.full(n, -1, np.int64)
    root[mem] = mem[comp]
    return root, int(adj.sum()) // 2


def check(fr, radius, what):
    got = GM.groups(fr, radius)
    root, nlinks = brute_roots(fr, radius)
    assert np.array_equal(got["root"], root), what
    assert got["links"] == nlinks, what
    size, first, group = got["group_size"], got["group_first"], got["group"]
    assert size.sum() == got["members"] == (root >= 0).sum() and got["singles"] == (size == 1).sum(), what
    assert got["largest"] == (size.max() if len(size) else 0) and got["groups"] == len(size) == len(first), what
    assert (np.diff(first) > 0).all(), what + ": group_first is not strictly ascending"
    assert np.array_equal(np.bincount(group[group >= 0], minlength=len(size)), size), what
    assert np.array_equal(first[group[group >= 0]], root[got["ids"][group >= 0]]), what
    assert ((group >= 0) == (root[got["ids"]] >= 0)).all() and got["unfinished"] == 0, what
    return got


@pytest.mark.parametrize("G", [4, 9])
def test_the_rough_cloud_equals_the_brute_force_and_has_its_shapes(G):
    fr = rough(G)
    small = check(fr, 0.4, "rough cloud, G = %d, radius 0.4" % G)
    big = check(fr, CS, "rough cloud, G = %d, radius cell_size" % G)
    print("G = %d: %d members; radius 0.4: %d groups, %d of two or more, largest %d; cell_size: %d groups, largest %d"
          % (G, small["members"], small["groups"], (small["group_size"] >= 2).sum(), small["largest"], big["groups"], big["largest"]))
    assert (small["group_size"] >= 2).sum() >= 20
    kids = fr.kid[small["ids"]]
    assert kids.any() and (small["group"][kids] == -1).all() and (small["group"][~kids] >= 0).all()
    over = SPECIAL["over"]
    assert fr.count[(over[2] * G + over[0]) * G + over[1]] == fr.cap and len(fr.live) < len(fr.filled), "no full-capacity cell"
    assert 2 * big["largest"] > big["members"]
    # the forms: a capacity cuts group[], a group_capacity the tables, the index form names group_first by export index
    for capacity in (0, 1, len(fr.live) // 3):
        short = GM.groups(fr, 0.4, capacity=capacity)
        assert np.array_equal(short["group"], small["group"][:capacity]) and np.array_equal(short["group_size"], small["group_size"])
    for room in (0, 1, small["groups"] - 1):
        short = GM.groups(fr, 0.4, group_capacity=room)
        assert np.array_equal(short["group_first"], small["group_first"][:room]) and np.array_equal(short["group"], small["group"])
        assert short["groups"] == small["groups"]
    by = GM.groups(fr, 0.4, index=True)
    assert np.array_equal(small["ids"][by["group_first"]], small["group_first"]) and np.array_equal(by["group"], small["group"])


def test_a_cloud_without_kids_links_every_directed_pair_twice():
    fr = rough(4, kids=False)
    for radius in (0.4, CS):
        got = check(fr, radius, "no kids, radius %g" % radius)
        assert 2 * got["links"] == M.neighbours(fr, radius)["pairs"] > 0


def test_the_snake_is_one_group_and_falls_apart_below_its_spacing():
    fr = snake_frame()
    n = len(fr.chain)
    assert 900 <= n <= 1200 and len(fr.live) == n
    one = check(fr, 0.4, "snake at 0.4")
    assert (one["groups"], one["largest"], one["links"]) == (1, n, n - 1)
    at = int(np.nonzero(fr.chain == fr.chain.min())[0][0])
    assert n // 10 < at < n - n // 10, "the smallest slot is near an end of the chain: %d of %d" % (at, n)
    apart = check(fr, 0.29, "snake at 0.29")
    assert (apart["groups"], apart["singles"], apart["links"]) == (n, n, 0)


def test_the_broken_snake_is_two_groups():
    cut = 30
    fr = snake_frame(cut)
    n = len(fr.chain)
    got = check(fr, 0.4, "broken snake")
    assert got["groups"] == 2 and sorted(got["group_size"].tolist()) == [cut, n - cut] and got["links"] == n - 2
    root = got["root"]
    assert len(set(root[fr.chain[:cut]])) == 1 and len(set(root[fr.chain[cut:]])) == 1


def test_the_near_miss_chains_join_at_the_next_radius():
    fr, radius = near_miss_frame()
    r = np.float32(radius)
    nxt = np.nextafter(r, np.float32(9))
    a, b = fr.filled[2], fr.filled[5]
    d2 = M.d2_fp32(fr.xyz[a:a + 1], fr.xyz[b:b + 1])[0, 0]
    assert np.nextafter(np.float32(r * r), np.float32(9)) == d2 and np.float32(nxt * nxt) >= d2, "the closest pair is not one ulp above r2"
    apart = check(fr, float(r), "near miss")
    assert apart["groups"] == 2 and apart["group_size"].tolist() == [5, 5] and apart["links"] == 8
    joined = check(fr, float(nxt), "near miss, the next radius")
    assert joined["groups"] == 1 and joined["largest"] == 10 and joined["links"] == 9


def test_the_dense_clump_is_one_group():
    fr = clump_frame()
    got = check(fr, 0.4, "clump")
    assert len(fr.cells()) == 1 and (got["groups"], got["largest"], got["links"]) == (1, 200, 200 * 199 // 2)


def test_members_with_a_non_finite_coordinate_and_particles_in_no_list():
    fr = M.Frame.__new__(M.Frame)
    fr.__dict__.update(rough(4).__dict__)
    fr.xyz = fr.xyz.copy()
    adult = np.nonzero(GM.members(fr))[0]
    fr.xyz[adult[5], 1] = np.nan
    fr.xyz[adult[6], 0] = np.inf
    fr.live = np.concatenate([fr.live, [len(fr.xyz)]])          # one more live slot that is in no list of the frame
    fr.xyz = np.concatenate([fr.xyz, [[0.0, 0.0, 0.0]]]).astype(np.float32)
    fr.kid = np.concatenate([fr.kid, [False]])
    got = GM.groups(fr, CS)
    at = {int(i): k for k, i in enumerate(got["ids"])}
    for i in adult[5:7]:
        g = got["group"][at[int(i)]]
        assert g >= 0 and got["group_size"][g] == 1 and got["group_first"][g] == i
    assert got["group"][-1] == -1 and got["members"] == len(adult)


def test_the_header_and_the_python_mirror_agree():
    """fails without the service: the header declares the functions and both struct sizes, the mirror's sizes agree, the
    library exports the symbols"""
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "psamd.h")).read()
    assert re.search(r"\bint psamd_groups\(psamd_ctx \*ctx, const psamd_groups_spec \*spec\);", text)
    assert re.search(r"\bint psamd_groups_result_get\(psamd_ctx \*ctx, psamd_groups_result \*out\);", text)
    assert re.search(r"\bint psamd_download_groups\(psamd_ctx \*ctx, uint32_t flags, float radius, int32_t \*group, int64_t capacity,", text)
    assert re.search(r"\}\s*psamd_groups_spec;\s*/\* 56 bytes \*/", text) and re.search(r"\}\s*psamd_groups_result;\s*/\* 40 bytes \*/", text)
    assert "#define PSAMD_GROUPS_INDEX 0x1u" in text and ps.GROUPS_INDEX == 1
    assert "#define PSAMD_ABI_VERSION 8" in text and ps.ABI_VERSION == 8
    assert C.sizeof(ps.GroupsSpec) == 56 and C.sizeof(ps.GroupsResult) == 40
    assert ps.GroupsSpec.capacity.offset == 16 and ps.GroupsSpec.group_capacity.offset == 40 and ps.GroupsSpec.result_dev.offset == 48
    assert ps.GroupsResult.largest.offset == 32 and ps.GroupsResult.unfinished.offset == 36
    names = {row[0] for row in ps.ABI}
    assert {"psamd_groups", "psamd_groups_result_get", "psamd_download_groups"} <= names
    lib = ps.load()
    assert lib.psamd_abi_version() == 8 and all(hasattr(lib, n) for n in names)
    for f in ("groups", "groups_result", "download_groups"):
        assert callable(getattr(ps.ParticleSystem, f))
