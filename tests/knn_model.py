"""psamd_knn in numpy (include/psamd.h, "the k nearest within a radius"): what test_knn_cpu.py holds against an fp64 brute
force and test_gpu_knn.py holds the device to, byte for byte.

The frame, the candidates and the fp32 d2 are neighbours_model's (Frame, candidates, d2_fp32): psamd_neighbours' rules are not
restated here.  What is new is the order: per query the hits sorted by (d2 as an fp32 value, global slot id) with np.lexsort,
the first k of them the row."""
import numpy as np

import neighbours_model as M

INF = M.INF
RECORD = ("listed", "found_sum", "full", "k", "dk2_min", "dk2_max")


def knn(fr, radius, k, capacity=None, index=False):
    """The service's outputs on the frame: {"ids": the live ids (the export order), "found" [m], "who" [m, k], "d2" [m, k], and
    the record's "listed", "found_sum" (the record's `found`: the array has the name, as in ParticleSystem.knn), "full", "k",
    "dk2_min", "dk2_max"}, the arrays cut to m = min(live, capacity).  "count": per slot id psamd_neighbours' count (-1: in no
    list), every query's."""
    k = int(k)
    r2 = np.float32(np.float32(radius) * np.float32(radius))
    n = len(fr.xyz)
    count = np.full(n, -1, np.int64)
    who = np.full((n, k), -1, np.int64)
    d2k = np.full((n, k), INF, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in fr.cells():
            q = fr.lists[c]
            cand = fr.candidates(c)
            d2 = M.d2_fp32(fr.xyz[q], fr.xyz[cand])
            hit = (d2 <= r2) & (cand[None, :] != q[:, None])          # (an id stands in one list once: by id is by sorted index)
            count[q] = hit.sum(1)
            for row, i in enumerate(q):
                ids, dist = cand[hit[row]], d2[row][hit[row]]
                order = np.lexsort((ids, dist))[:k]                     # by d2, ties by id
                who[i, :len(order)] = ids[order]
                d2k[i, :len(order)] = dist[order]
    queries = np.concatenate([fr.lists[c] for c in fr.cells()] or [np.zeros(0, np.int64)])
    ids = fr.live
    m = len(ids) if capacity is None else min(len(ids), int(capacity))
    ids_m = ids[:m]
    rank = np.full(n, -1, np.int64)
    rank[ids] = np.arange(len(ids))
    names = who[ids_m]
    if index:
        names = np.where(names >= 0, rank[np.maximum(names, 0)], -1)
    cq = count[queries]
    full = cq >= k
    kth = d2k[queries][full, k - 1]
    return {"ids": ids_m.astype(np.int32), "found": np.where(count[ids_m] < 0, -1, np.minimum(count[ids_m], k)).astype(np.int32),
            "who": names.astype(np.int32).reshape(m, k), "d2": d2k[ids_m].reshape(m, k), "count": count,
            "listed": int(len(queries)), "found_sum": int(np.minimum(cq, k).sum()), "full": int(full.sum()), "k": k,
            "dk2_min": float(kth.min()) if len(kth) else float("inf"), "dk2_max": float(kth.max()) if len(kth) else float("-inf")}


def brute_rows(fr, radius, k):
    """fp64 over the same stencil: per query id the ids of its k nearest within the radius by (exact distance, id)"""
    rows = {}
    xyz = fr.xyz.astype(np.float64)
    for c in fr.cells():
        q = fr.lists[c]
        cand = fr.candidates(c)
        r = xyz[cand][None, :, :] - xyz[q][:, None, :]
        dist2 = (r * r).sum(2)
        hit = (dist2 <= float(radius) ** 2) & (cand[None, :] != q[:, None])
        for row, i in enumerate(q):
            ids, d = cand[hit[row]], dist2[row][hit[row]]
            order = sorted(range(len(ids)), key=lambda j: (d[j], ids[j]))[:k]
            rows[int(i)] = (ids[order], d[order])
    return rows


# ---- clouds test_gpu_knn.py runs and test_knn_cpu.py holds to their shapes (xyz in a 4^3 grid of 5-unit cells: the box is
# [-10, 10)^3 and the cell walls are the multiples of 5; every coordinate a multiple of 2^-13 or coarser, so every d2 is exact)

def tie_lattice(straddle, seed=3):
    """a 5 x 5 x 5 unit cubic lattice in a shuffled row order: inside one cell, or -- straddle -- across the wall at 5 on every
    axis, so that tied candidates come from different stencil cells.  At radius 1.5 an interior point has 6 neighbours at
    d2 = 1 and 12 at d2 = 2.  Returns (xyz, interior: the rows of the 27 interior points)."""
    base = 2.75 if straddle else 0.25
    i = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing="ij"), -1).reshape(-1, 3)
    order = np.random.default_rng(seed).permutation(len(i))
    i = i[order]
    interior = np.nonzero(((i >= 1) & (i <= 3)).all(1))[0]
    return (base + i).astype(np.float32), interior


LINE = 73           # the bodies of a line beside its query: more than a slice of 64, more than twice the largest k


def line(far_first, spread):
    """a query and LINE bodies at growing distances from it, 1/16 apart along x: in one cell, or -- spread -- on a slant that
    crosses the wall at x = 5 and then the wall at y = 5, three cells of the query's stencil.  Row order (inside a cell rows fill ascending slots): the
    query last and the bodies from far to near (every hit displaces the whole row), or the query first and the bodies from
    near to far (every hit after the k-th is rejected).  Returns (xyz, query row, rows of the bodies from near to far)."""
    t = np.arange(LINE + 1) / 16.0
    if spread:
        xyz = np.stack([4.0 + t, 4.5 + t / 4.0, np.full_like(t, 2.5)], 1)
    else:
        xyz = np.stack([0.25 + t, np.full_like(t, 2.5), np.full_like(t, 2.5)], 1)
    rows = np.arange(LINE + 1)
    if far_first:
        xyz, rows = xyz[::-1], rows[::-1]
    query = int(np.nonzero(rows == 0)[0][0])
    near_to_far = np.argsort(rows)[1:]
    return np.ascontiguousarray(xyz, np.float32), query, near_to_far


def ulp_pair(near_first):
    """a query at (1, 1, 1) and two bodies of its cell whose d2 differ by one ulp: 0.5625 and 0.5625 + 2^-24.  Rows: query, then the
    nearer body first (it has the lower id) or the farther one first.  Returns (xyz, query row, nearer row, farther row)."""
    near, far = (1.75, 1.0, 1.0), (1.75, 1.0 + 2.0 ** -12, 1.0)
    xyz = np.array([(1.0, 1.0, 1.0)] + ([near, far] if near_first else [far, near]), np.float32)
    return xyz, 0, 1 if near_first else 2, 2 if near_first else 1
