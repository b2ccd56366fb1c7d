"""psamd_groups in numpy (include/psamd.h, "groups within a radius"): what test_groups_cpu.py holds against a brute force and
test_gpu_groups.py holds the device to, byte for byte.  Built on neighbours_model's Frame, stencil and d2_fp32: the members are
its candidates seen as queries, the links its test, each undirected pair once; the components come from a plain serial
union-find.

Also the clouds both test files use on the 4^3 grid of 5-unit cells (the box is [-10, 10)^3): the snake, the near-miss chains
and the dense clump.  They are here, not in a test file, so that the shapes the CPU test asserts are the shapes the GPU test
runs."""
import numpy as np

import neighbours_model as M


def members(fr):
    """bool per slot: a listed particle that is no kid"""
    m = np.zeros(len(fr.xyz), bool)
    for c in fr.cells():
        m[fr.lists[c]] = True
    return m & ~fr.kid


def links(fr, radius):
    """[n, 2] int64: every undirected link once, the higher slot first"""
    r2 = np.float32(np.float32(radius) * np.float32(radius))
    out = [np.zeros((0, 2), np.int64)]
    with np.errstate(invalid="ignore", over="ignore"):
        for c in fr.cells():
            q = fr.lists[c]
            q = q[~fr.kid[q]]
            cand = fr.candidates(c)
            if not len(q) or not len(cand):
                continue
            hit = (M.d2_fp32(fr.xyz[q], fr.xyz[cand]) <= r2) & (cand[None, :] < q[:, None])      # (a < b: not the own entry)
            a, b = np.nonzero(hit)
            out.append(np.stack([q[a], cand[b]], 1))
    return np.concatenate(out)


def components(n, pairs):
    """the smallest slot of every slot's set, by a serial union-find (path halving, the smaller root wins)"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in pairs.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(n)], np.int64)


def groups(fr, radius, capacity=None, group_capacity=None, index=False):
    """The service's outputs on the frame: {"ids": the live ids (the export order), "group", "group_first", "group_size", and
    the record's "members", "groups", "links", "singles", "largest", "unfinished"}; group cut to m = min(live, capacity), the
    tables to min(groups, group_capacity).  "root": per slot its group's smallest slot (-1: no member)."""
    n = len(fr.xyz)
    mem = members(fr)
    pairs = links(fr, radius)
    root = np.where(mem, components(n, pairs), -1)
    firsts, inverse, sizes = np.unique(root[mem], return_inverse=True, return_counts=True)       # ascending slot id
    number = np.full(n, -1, np.int64)
    number[np.nonzero(mem)[0]] = inverse
    ids = fr.live
    m = len(ids) if capacity is None else min(len(ids), int(capacity))
    ng = len(firsts) if group_capacity is None else min(len(firsts), int(group_capacity))
    rank = np.full(n, -1, np.int64)
    rank[ids] = np.arange(len(ids))
    first = rank[firsts] if index else firsts
    return {"ids": ids[:m].astype(np.int32), "group": number[ids[:m]].astype(np.int32), "group_first": first[:ng].astype(np.int32),
            "group_size": sizes[:ng].astype(np.int32), "root": root,
            "members": int(mem.sum()), "groups": int(len(firsts)), "links": int(len(pairs)), "singles": int((sizes == 1).sum()),
            "largest": int(sizes.max()) if len(sizes) else 0, "unfinished": 0}


# ---- the rough cloud ---------------------------------------------------------------------------------------------------------------

def rough_groups_cloud(G, cap, seed=17):
    """(xyz, age): test_gpu_neighbours' rough_cloud -- the special cells, kids, an over-age particle, twins, a pair across a
    wall -- and, because its background of six per cell holds few pairs within 0.4, forty small knots of adults (two to five
    points 0.25 apart in a row) at random places outside the special cells: groups of two or more at radius 0.4."""
    from test_gpu_neighbours import CS, SPECIAL, cell_of, rough_cloud
    xyz, age = rough_cloud(G, cap)
    rng = np.random.default_rng(seed + G)
    special = [(c[2] * G + c[0]) * G + c[1] for c in SPECIAL.values()]
    lo, hi = -(G // 2) * CS, (G - G // 2) * CS
    knots = []
    while len(knots) < 40:
        n = int(rng.integers(2, 6))
        q = rng.uniform(lo + 1.5, hi - 1.5, 3)[None, :] + 0.25 * np.arange(n)[:, None] * np.eye(3)[rng.integers(0, 3)][None, :]
        p = np.stack([q[:, 1], -q[:, 0], -q[:, 2]], 1).astype(np.float32)       # the cell axes are (-y, x, -z)
        if not np.isin(cell_of(G, p), special).any():
            knots.append(p)
    extra = np.concatenate(knots)
    return np.concatenate([xyz, extra]).astype(np.float32), np.concatenate([age, np.full(len(extra), 3.0, np.float32)])


# ---- clouds on the 4^3 grid ------------------------------------------------------------------------------------------------------

STEP = 0.3


def snake(gap_at=None, gap=0.41, seed=3):
    """(xyz in shuffled order, chain: the row of xyz that holds the chain's k-th point).  One chain on the lattice of STEP: 16
    x-rows of 57 points, eight to each of two cell layers (z = -2.4 and 2.4), joined at their ends -- consecutive points are
    STEP apart along one axis, any two points at least STEP.  gap_at: the chain is cut between its points gap_at - 1 and
    gap_at (inside the first row, which runs along +x) and everything from gap_at on is moved by gap - STEP along x."""
    pts = []
    ks = list(range(-28, 29))
    js = list(range(-28, 29, 8))                      # the rows' y, 2.4 apart: 8 rows, two to each row of cells
    fwd = True
    for layer, l in enumerate((-8, 8)):
        for r, j in enumerate(js if layer == 0 else js[::-1]):
            row = ks if fwd else ks[::-1]
            if pts:                                   # the way from the last point: along z between the layers, along y inside one
                k0, j0, l0 = pts[-1]
                if l0 != l:
                    pts += [(k0, j0, v) for v in range(l0 + 1, l)]
                else:
                    s = 1 if j > j0 else -1
                    pts += [(k0, v, l0) for v in range(j0 + s, j, s)]
            pts += [(k, j, l) for k in row]
            fwd = not fwd
    xyz = (np.array(pts, np.float64) * STEP)
    if gap_at is not None:
        assert 0 < gap_at < len(ks)
        xyz[gap_at:, 0] += gap - STEP
    xyz = xyz.astype(np.float32)
    order = np.random.default_rng(seed).permutation(len(xyz))
    chain = np.empty(len(xyz), np.int64)
    chain[order] = np.arange(len(xyz))                # xyz[order][chain[k]] is the chain's k-th point
    return xyz[order], chain


def near_miss(base=(1.0, 1.0, 1.0)):
    """(xyz, radius): two chains of five points STEP apart, the first (rows 0-4) along x, the second (rows 5-9) leaving from
    beside the first's middle along y, whose closest pair -- rows 2 and 5 -- has an fp32 d2 exactly one ulp above r2 = RN(radius radius), and at or below RN(next next) for next = nextafter(radius).
    The second chain's offset is scanned until a radius with that property exists; the radius is the model's answer (the
    largest fp32 whose square rounds below d2), never a constant."""
    base = np.asarray(base, np.float32)
    a = base[None, :] + np.array([[STEP * k, 0.0, 0.0] for k in range(-2, 3)], np.float32)
    for t in range(4096):
        off = np.array([np.float32(0.1), np.float32(0.39) + np.float32(t) * np.float32(2.0 ** -24), 0.0], np.float32)
        b = (a[2] + off)[None, :] + np.array([[0.0, STEP * k, 0.0] for k in range(5)], np.float32)
        b = b.astype(np.float32)
        d2 = M.d2_fp32(a[2:3], b[0:1])[0, 0]
        r = np.float32(np.sqrt(np.float64(d2)))
        while np.float32(r * r) >= d2:
            r = np.nextafter(r, np.float32(0))
        while np.float32(np.nextafter(r, np.float32(1)) * np.nextafter(r, np.float32(1))) < d2:
            r = np.nextafter(r, np.float32(1))
        if np.nextafter(np.float32(r * r), np.float32(1)) == d2:
            return np.concatenate([a, b]).astype(np.float32), float(r)
    raise AssertionError("no offset gives a near miss")


def clump(n=200, centre=(2.5, 2.5, 2.5), seed=9):
    """n points inside a ball of diameter 0.3 in the middle of one cell: every pair is within 0.4"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v *= (0.15 * rng.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
    return (np.asarray(centre)[None, :] + v).astype(np.float32)
