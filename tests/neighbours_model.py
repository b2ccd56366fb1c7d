"""psamd_neighbours in numpy (include/psamd.h, "neighbours within a radius"): what test_neighbours_cpu.py holds against an fp64
brute force and test_gpu_neighbours.py holds the device to, byte for byte.

Inputs are a context's downloaded particles (or the oracle's: the same records) and cell grid -- ids ascending in a cell,
truncated at the list capacity -- plus the geometry.  A slot's id is its index in the particle array.

The stencil's order is the reference's, taken from the oracle's pso_fill_cells (the own cell first, then the 26 candidates in
the order fill_cells probes them); it is not restated here."""
import ctypes as C
import functools

import numpy as np

import oracle_py as O

INF = np.float32(np.inf)


@functools.lru_cache(maxsize=None)
def stencil(c, G):
    """the cells of c's non-periodic stencil in the reference's order, c first"""
    out = (C.c_int * 27)()
    n = O.lib().pso_fill_cells(C.byref(O.Derived(grid_dim=int(G))), int(c), out)
    return tuple(out[k] for k in range(n))


class Frame:
    """the lists, the kids and the positions of a built frame"""

    def __init__(self, p, cg, G, kid_age, max_per_cell=None):
        self.G, self.num_cells = int(G), int(G) ** 3
        cap = cg.shape[1] - 1 if max_per_cell is None else int(max_per_cell)
        self.count = np.minimum(cg[:, 0], cap).astype(np.int64)
        self.lists = [np.asarray(cg[c, 1:1 + self.count[c]], np.int64) for c in range(self.num_cells)]
        self.xyz = np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float32)
        self.kid = p["age"].astype(np.float64) < kid_age
        self.live = np.nonzero((p["cell"] >= 0) & (p["cell"] < self.num_cells))[0]       # the export order: ascending slot id

    def cells(self):
        return np.nonzero(self.count)[0]

    def candidates(self, c):
        """the bodies every query of cell c is tested against, in walk order: no kids"""
        cand = np.concatenate([self.lists[k] for k in stencil(int(c), self.G)])
        return cand[~self.kid[cand]]


def d2_fp32(xi, xj):
    """[queries, candidates] float32: RN(RN(RN(rx rx) + RN(ry ry)) + RN(rz rz)), every step rounded to fp32 on its own"""
    r = (xj[None, :, :] - xi[:, None, :]).astype(np.float32)
    sq = (r * r).astype(np.float32)
    return ((sq[:, :, 0] + sq[:, :, 1]).astype(np.float32) + sq[:, :, 2]).astype(np.float32)


def neighbours(fr, radius, capacity=None, index=False):
    """The service's outputs on the frame: {"ids": the live ids (the export order), "count", "nearest", "nearest_d2", "offsets",
    "list", and the record's "listed", "pairs", "wanted", "max_count", "d2_min"}, the arrays cut to m = min(live, capacity).
    "lists": per slot id the neighbours' ids in walk order (a dict, every query's)."""
    r2 = np.float32(np.float32(radius) * np.float32(radius))
    n = len(fr.xyz)
    count = np.full(n, -1, np.int32)
    near = np.full(n, -1, np.int32)
    near_d2 = np.full(n, INF, np.float32)
    lists = {}
    with np.errstate(invalid="ignore", over="ignore"):
        for c in fr.cells():
            q = fr.lists[c]
            cand = fr.candidates(c)
            d2 = d2_fp32(fr.xyz[q], fr.xyz[cand])
            hit = (d2 <= r2) & (cand[None, :] != q[:, None])          # (an id stands in one list once: by id is by sorted index)
            count[q] = hit.sum(1)
            d = np.where(hit, d2, INF)
            dmin = d.min(1) if len(cand) else np.full(len(q), INF, np.float32)
            tie = hit & (d2 == dmin[:, None])
            who = np.where(tie, cand[None, :], np.iinfo(np.int64).max).min(1) if len(cand) else np.full(len(q), -1)
            some = hit.any(1)
            near[q] = np.where(some, who, -1)
            near_d2[q] = np.where(some, dmin, INF)
            for k, i in enumerate(q):
                lists[int(i)] = cand[hit[k]].astype(np.int32)
    queries = np.concatenate([fr.lists[c] for c in fr.cells()] or [np.zeros(0, np.int64)])
    ids = fr.live
    m = len(ids) if capacity is None else min(len(ids), int(capacity))
    ids_m = ids[:m]
    offsets = np.zeros(m + 1, np.int64)
    offsets[1:] = np.cumsum(np.maximum(count[ids_m], 0))
    rank = np.full(n, -1, np.int64)
    rank[ids] = np.arange(len(ids))
    name = (lambda a: rank[a].astype(np.int32)) if index else (lambda a: np.asarray(a, np.int32))
    empty = np.zeros(0, np.int32)
    flat = np.concatenate([name(lists.get(int(i), empty)) for i in ids_m] or [empty]).astype(np.int32)
    near_m = near[ids_m]
    return {"ids": ids_m.astype(np.int32), "count": count[ids_m], "nearest": np.where(near_m >= 0, name(np.maximum(near_m, 0)), -1).astype(np.int32),
            "nearest_d2": near_d2[ids_m], "offsets": offsets, "list": flat, "lists": lists,
            "listed": int(len(queries)), "pairs": int(count[queries].sum()), "wanted": int(offsets[m]),
            "max_count": int(count[queries].max()) if len(queries) else 0,
            "d2_min": float(near_d2[queries].min()) if len(queries) else float("inf")}


def brute_sets(fr, radius):
    """fp64 over the same stencil, no pair left out: per query id the set of neighbour ids, and the fp64 distance of every
    candidate pair as (query, candidate, dist) arrays"""
    sets, qq, cc, dd = {}, [], [], []
    xyz = fr.xyz.astype(np.float64)
    for c in fr.cells():
        q = fr.lists[c]
        cand = fr.candidates(c)
        r = xyz[cand][None, :, :] - xyz[q][:, None, :]
        dist = np.sqrt((r * r).sum(2))
        other = cand[None, :] != q[:, None]
        hit = (dist <= float(radius)) & other
        for k, i in enumerate(q):
            sets[int(i)] = set(cand[hit[k]].tolist())
        a, b = np.nonzero(other)
        qq.append(q[a]); cc.append(cand[b]); dd.append(dist[a, b])
    return sets, np.concatenate(qq), np.concatenate(cc), np.concatenate(dd)
