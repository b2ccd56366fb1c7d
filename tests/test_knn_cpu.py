"""The numpy model of psamd_knn (tests/knn_model.py) against an fp64 brute-force ordering, its own invariants, the shapes of
the clouds test_gpu_knn.py runs, and the header's declarations.  No GPU: the frames are the oracle's (fill, init_iframe,
build_grid), whose particle records and cell grid are what a context downloads.

Exactness.  The lattice clouds are test_neighbours_cpu's: every coordinate a multiple of 2^-6 inside +-20.  Its argument shows
that every fp32 d2 that is <= r2 (r2 <= 25) is exact there, so the model's order by (fp32 d2, id) must be the fp64 order by
(exact d2, id) with no row left out: rows are compared as they stand, there is no tolerance."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import knn_model as KM
import neighbours_model as M
import oracle_py as O
import particlesystem_amd as ps
from test_groups_cpu import adults, frame
from test_gpu_neighbours import CS, GRIDS, rough_cloud
from test_neighbours_cpu import ages, frame as frame8, lattice_cloud

KS = (1, 7, 8, 9, 32)                            # what test_gpu_knn.py asks for: both sides of a tier edge, and the maximum
RADII = (CS, 0.4)


def same_rows(got, want, what):
    for key in ("found", "who"):
        assert np.array_equal(got[key], want[key]), (what, key)
    assert np.array_equal(got["d2"].view(np.uint32), want["d2"].view(np.uint32)), (what, "d2")


@functools.lru_cache(maxsize=None)
def lattice_frame():
    xyz = np.concatenate([lattice_cloud(3000, 1), lattice_cloud(600, 2, 2.0, 10.0)])       # a dense blob inside a chunk: full rows of 32 at radius 1
    return frame8(xyz, ages(len(xyz), 3), max_particles_num=1 << 18)


@pytest.mark.parametrize("radius", [5.0, 1.0])
def test_lattice_clouds_equal_the_fp64_ordering(radius):
    fr = lattice_frame()
    for k in (1, 7, 32):
        got = KM.knn(fr, radius, k)
        want = KM.brute_rows(fr, radius, k)
        assert got["listed"] == len(want) == len(fr.live)
        at = {int(i): p for p, i in enumerate(got["ids"])}
        full = 0
        for i, (ids, d) in want.items():
            p, n = at[i], len(ids)
            assert got["found"][p] == n, (radius, k, i)
            assert np.array_equal(got["who"][p, :n], ids) and (got["who"][p, n:] == -1).all(), (radius, k, i)
            assert np.array_equal(got["d2"][p, :n].astype(np.float64), d) and np.isposinf(got["d2"][p, n:]).all(), (radius, k, i)
            full += n == k
        assert full > 100 and got["found_sum"] == sum(len(ids) for ids, _ in want.values())


@functools.lru_cache(maxsize=None)
def rough(G):
    o = O.System(O.default_config(**GRIDS[G]))
    cap = int(o.d.max_per_cell)
    o.close()
    xyz, age = rough_cloud(G, cap)
    return frame(xyz, age, G)


def test_invariants():
    fr = rough(4)
    for radius in RADII:
        nb = M.neighbours(fr, radius)
        big = KM.knn(fr, radius, 32)
        assert np.array_equal(big["ids"], nb["ids"])
        for k in KS:
            got = KM.knn(fr, radius, k)
            what = "radius %g, k = %d" % (radius, k)
            assert np.array_equal(got["who"], big["who"][:, :k]) and np.array_equal(got["d2"].view(np.uint32), big["d2"][:, :k].view(np.uint32)), what
            assert np.array_equal(got["found"], np.where(nb["count"] < 0, -1, np.minimum(nb["count"], k))), what
            # the words past found, and only they, are -1 / +inf; a row ascends by (d2, id)
            past = np.arange(k)[None, :] >= np.maximum(got["found"], 0)[:, None]
            assert np.array_equal(got["who"] == -1, past) and np.array_equal(np.isposinf(got["d2"]), past), what
            d, w = got["d2"][:, :-1], got["who"][:, :-1]
            ok = past[:, 1:] | (d < got["d2"][:, 1:]) | ((d == got["d2"][:, 1:]) & (w < got["who"][:, 1:]))
            assert ok.all(), what
            # the record's sums agree with the arrays (every live particle of this frame is a query)
            f = got["found"]
            assert got["listed"] == nb["listed"] == len(f) and got["found_sum"] == f.sum() and got["full"] == (nb["count"] >= k).sum() and got["k"] == k, what
            kth = got["d2"][f == k, k - 1]
            assert got["dk2_min"] == float(kth.min(initial=np.inf)) and got["dk2_max"] == float(kth.max(initial=-np.inf)), what
        one = KM.knn(fr, radius, 1)
        assert np.array_equal(one["who"][:, 0], nb["nearest"]) and np.array_equal(one["d2"][:, 0].view(np.uint32), nb["nearest_d2"].view(np.uint32))
        # a capacity cuts the arrays and not the record; the index form names through the export order
        short = KM.knn(fr, radius, 7, capacity=len(fr.live) // 3)
        whole = KM.knn(fr, radius, 7)
        same_rows(short, {key: whole[key][:len(fr.live) // 3] for key in ("found", "who", "d2")}, "capacity")
        assert {key: short[key] for key in KM.RECORD} == {key: whole[key] for key in KM.RECORD}
        by = KM.knn(fr, radius, 7, index=True)
        has = by["who"] >= 0
        assert np.array_equal(has, whole["who"] >= 0) and np.array_equal(whole["ids"][by["who"][has]], whole["who"][has])
    none = KM.knn(fr, 1e-4, 3)
    assert none["full"] == 0 and none["dk2_min"] == float("inf") and none["dk2_max"] == float("-inf") and none["found_sum"] > 0     # (the twins)


@pytest.mark.parametrize("G", [4, 9])
def test_the_rough_cloud_has_every_shape_of_a_row(G):
    """Per k, over the two radii of the GPU tests: empty rows, rows cut by the radius (k > 1), and full rows -- exactly full or
    cut by k.  Radius 0.4 has the empty and the short rows, cell_size the full ones; which radius holds which is printed."""
    fr = rough(G)
    for k in KS:
        seen = set()
        for radius in RADII:
            got = KM.knn(fr, radius, k)
            count = got["count"][got["ids"]]
            here = {"empty": (got["found"] == 0).any(), "short": ((got["found"] > 0) & (got["found"] < k)).any(),
                    "exact": (count == k).any(), "cut": (count > k).any()}
            print("G = %d, k = %d, radius %g: %s; full %d of %d" % (G, k, radius, sorted(n for n, v in here.items() if v), got["full"], got["listed"]))
            seen |= {n for n, v in here.items() if v}
            assert got["who"].shape == (len(fr.live), k) and fr.kid[got["ids"]].any() and not fr.kid[got["who"][got["who"] >= 0]].any()
        assert "empty" in seen and ("exact" in seen or "cut" in seen) and ("short" in seen or k == 1), (G, k, seen)
    # found == -1: a live slot that is in no list of the frame (the model's own case, as in test_neighbours_cpu)
    more = M.Frame.__new__(M.Frame)
    more.__dict__.update(fr.__dict__)
    more.live = np.concatenate([fr.live, [len(fr.xyz)]])
    more.xyz = np.concatenate([fr.xyz, [[0.0, 0.0, 0.0]]]).astype(np.float32)
    more.kid = np.concatenate([fr.kid, [False]])
    got = KM.knn(more, CS, 7)
    assert got["found"][-1] == -1 and (got["who"][-1] == -1).all() and np.isposinf(got["d2"][-1]).all() and (got["found"][:-1] >= 0).all()
    assert got["listed"] == len(fr.live) and KM.knn(more, CS, 7, capacity=len(fr.live))["found"].min() >= 0


def test_the_tie_lattices_cut_inside_a_shell():
    for straddle in (False, True):
        xyz, interior = KM.tie_lattice(straddle)
        fr = frame(xyz, adults(xyz))
        slots = fr.filled
        cells = len(fr.cells())
        assert cells == (8 if straddle else 1) and not (np.diff(slots[np.argsort(xyz[:, 0], kind="stable")]) > 0).all()
        at = {int(i): p for p, i in enumerate(fr.live)}
        r = xyz[:, None, :].astype(np.float64) - xyz[None, :, :]
        exact = (r * r).sum(2)
        for k, shell_d2, before in ((4, 1.0, 0), (8, 2.0, 6)):
            got = KM.knn(fr, 1.5, k)
            for row in interior:
                p = at[int(slots[row])]
                shell = np.sort(slots[exact[row] == shell_d2])
                assert len(shell) == (6 if shell_d2 == 1.0 else 12) and got["found"][p] == k
                assert np.array_equal(got["who"][p, before:], shell[:k - before]) and (got["d2"][p, before:] == shell_d2).all(), (straddle, k, row)
                assert np.array_equal(got["who"][p, :before], np.sort(slots[exact[row] == 1.0])[:before])


def test_the_lines_and_the_one_ulp_pair():
    cap = rough(4).cap
    for spread in (False, True):
        for far_first in (True, False):
            xyz, query, near_to_far = KM.line(far_first, spread)
            fr = frame(xyz, adults(xyz))
            assert len(xyz) == KM.LINE + 1 <= cap and KM.LINE >= 70
            assert len(fr.cells()) == (3 if spread else 1)
            got = KM.knn(fr, CS, 32)
            p = int(np.nonzero(got["ids"] == fr.filled[query])[0][0])
            assert got["count"][fr.filled[query]] == KM.LINE and np.array_equal(got["who"][p], fr.filled[near_to_far[:32]])
            assert (np.diff(got["d2"][p]) > 0).all()
            if not spread:                   # one cell: the list order is the slot order, the walk meets the line as laid out
                slot_order = fr.filled[near_to_far]
                assert (np.diff(slot_order) < 0).all() if far_first else (np.diff(slot_order) > 0).all()
                assert (fr.filled[query] > slot_order.max()) if far_first else (fr.filled[query] < slot_order.min())
    for near_first in (True, False):
        xyz, query, near, far = KM.ulp_pair(near_first)
        fr = frame(xyz, adults(xyz))
        assert (np.diff(fr.filled) > 0).all() and len(fr.cells()) == 1
        got = KM.knn(fr, CS, 2)
        p = int(np.nonzero(got["ids"] == fr.filled[query])[0][0])
        assert got["who"][p].tolist() == [fr.filled[near], fr.filled[far]] and (fr.filled[near] < fr.filled[far]) == near_first
        a, b = got["d2"][p]
        assert a == np.float32(0.5625) and b == np.nextafter(a, np.float32(1))


def test_the_header_and_the_python_mirror_agree():
    """fails without the service: the header declares the functions and both struct sizes, the mirror's sizes agree, the
    library exports the symbols"""
    here = os.path.dirname(os.path.abspath(__file__))
    text = open(os.path.join(here, "..", "include", "psamd.h")).read()
    assert re.search(r"\bint psamd_knn\(psamd_ctx \*ctx, const psamd_knn_spec \*spec\);", text)
    assert re.search(r"\bint psamd_knn_result_get\(psamd_ctx \*ctx, psamd_knn_result \*out\);", text)
    assert re.search(r"\bint psamd_download_knn\(psamd_ctx \*ctx, uint32_t flags, float radius, int32_t k, int32_t \*found, int32_t \*who, float \*d2,", text)
    assert re.search(r"\}\s*psamd_knn_spec;\s*/\* 56 bytes \*/", text) and re.search(r"\}\s*psamd_knn_result;\s*/\* 48 bytes \*/", text)
    assert "#define PSAMD_KNN_INDEX 0x1u" in text and ps.KNN_INDEX == 1
    assert re.search(r"#define PSAMD_KNN_MAX_K 32\b", text) and ps.KNN_MAX_K == 32
    assert "#define PSAMD_ABI_VERSION 8" in text and ps.ABI_VERSION == 8
    assert C.sizeof(ps.KnnSpec) == 56 and C.sizeof(ps.KnnResult) == 48
    assert ps.KnnSpec.k.offset == 8 and ps.KnnSpec.found.offset == 16 and ps.KnnSpec.capacity.offset == 40 and ps.KnnSpec.result_dev.offset == 48
    assert ps.KnnResult.k.offset == 24 and ps.KnnResult.dk2_min.offset == 32 and ps.KnnResult.dk2_max.offset == 40
    names = {row[0] for row in ps.ABI}
    assert {"psamd_knn", "psamd_knn_result_get", "psamd_download_knn"} <= names
    lib = ps.load()
    assert lib.psamd_abi_version() == 8 and all(hasattr(lib, n) for n in names)
    for f in ("knn", "knn_result", "download_knn"):
        assert callable(getattr(ps.ParticleSystem, f))
    assert callable(ps.merge_knn)
