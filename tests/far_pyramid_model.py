"""Far-field gravity from a pyramid of monopoles (PSAMD_FLAG_FAR_PYRAMID), restated in numpy from the definition in
include/psamd.h ("a pyramid of monopoles") -- not from the library's code.  Shared by test_far_pyramid_cpu.py,
test_gpu_far_pyramid.py and scripts/far_pyramid_cost.py.

Frames, lists and the numbering of cells are far_monopole_model.py's; a level-l cell is numbered (k3 * G_l + k1) * G_l + k2."""
import numpy as np

import far_monopole_model as M


def levels_of(G):
    """[G_0 .. G_L]: halved (rounded up) until at most 4"""
    dims = [int(G)]
    while dims[-1] > 4:
        dims.append((dims[-1] + 1) // 2)
    return dims


def coords(c, G):
    i3, rem = divmod(int(c), G * G)
    i1, i2 = divmod(rem, G)
    return i1, i2, i3


def level_sums(lists, xyz, w_eff, G):
    """per level float64 [G_l^3, 4] = (S, Sx, Sy, Sz).  Level 0: sequentially in list order (far_monopole_model.moments'
    sums).  Level l + 1: the existing children's sums added one at a time in ascending child index to +0 -- a child that does
    not exist is entered as +0 here, which leaves every bit as it is"""
    xyz = np.asarray(xyz, np.float32)
    w_eff = np.asarray(w_eff, np.float32)
    dims = levels_of(G)
    s0 = np.zeros((G ** 3, 4))
    for c, l in enumerate(lists):
        if len(l):
            w = w_eff[l].astype(np.float64)
            s0[c, 0] = np.cumsum(w)[-1]
            for k in range(3):
                s0[c, 1 + k] = np.cumsum(w * xyz[l, k].astype(np.float64))[-1]
    out = [s0]
    for lvl in range(1, len(dims)):
        Gc, Gp = dims[lvl - 1], dims[lvl]
        child = np.zeros((2 * Gp, 2 * Gp, 2 * Gp, 4))                 # [k3, k1, k2]
        child[:Gc, :Gc, :Gc] = out[-1].reshape(Gc, Gc, Gc, 4)
        acc = np.zeros((Gp, Gp, Gp, 4))
        for d3 in (0, 1):                                            # ascending child index: k3 slowest, k2 fastest
            for d1 in (0, 1):
                for d2 in (0, 1):
                    acc = acc + child[d3::2, d1::2, d2::2]
        out.append(acc.reshape(Gp ** 3, 4))
    return out


def level_moments(lists, xyz, w_eff, G):
    """per level float32 [G_l^3, 4] = (X, Y, Z, M): M = (float)S, X = (float)(Sx / S); S == 0: four zeros"""
    out = []
    for s in level_sums(lists, xyz, w_eff, G):
        m = np.zeros((len(s), 4), np.float32)
        nz = s[:, 0] != 0.0
        m[nz, :3] = (s[nz, 1:] / s[nz, :1]).astype(np.float32)
        m[nz, 3] = s[nz, 0].astype(np.float32)
        out.append(m)
    return out


def interaction_set(c, G):
    """[(level, level cell index)] of a particle in cell c: at the top level every cell not within 1 (max-norm) of c's; below
    it every cell whose parent is within 1 of c's parent and which is not itself within 1 of c's cell of that level"""
    dims = levels_of(G)
    L = len(dims) - 1
    i1, i2, i3 = coords(c, G)
    out = []
    for lvl in range(L, -1, -1):
        Gl = dims[lvl]
        a = (i1 >> lvl, i2 >> lvl, i3 >> lvl)
        if lvl == L:
            rng = [range(Gl)] * 3
        else:
            rng = [range(max(2 * ((x >> 1) - 1), 0), min(2 * ((x >> 1) + 1) + 2, Gl)) for x in a]
        j3, j1, j2 = np.meshgrid(np.array(rng[2]), np.array(rng[0]), np.array(rng[1]), indexing="ij")      # (index order)
        far = np.maximum(np.maximum(abs(j1 - a[0]), abs(j2 - a[1])), abs(j3 - a[2])) > 1
        out += [(lvl, int(J)) for J in ((j3 * Gl + j1) * Gl + j2)[far]]
    return out


def coverage(c, G, members=None):
    """int [G^3]: how often every cell of the box is covered -- by c's stencil, or by a member of c's set (as a leaf under it)"""
    n = np.zeros(G ** 3, np.int64)
    n[M.stencil_cells(c, G)] += 1
    cube = n.reshape(G, G, G)                                         # [i3, i1, i2]; i >> lvl == j: i in [j << lvl, (j + 1) << lvl)
    dims = levels_of(G)
    for lvl, J in (interaction_set(c, G) if members is None else members):
        j1, j2, j3 = coords(J, dims[lvl])
        cube[j3 << lvl:(j3 + 1) << lvl, j1 << lvl:(j1 + 1) << lvl, j2 << lvl:(j2 + 1) << lvl] += 1
    return n


def far_part(levmom, G, at, c, eps2):
    """fp64 acceleration at the points `at` [t, 3], all of cell c, from the members of c's set with the float32-rounded
    moments `levmom` (level_moments()); a member with M == 0 adds nothing"""
    members = interaction_set(c, G)
    m = np.array([levmom[lvl][J] for lvl, J in members], np.float64).reshape(-1, 4)
    m = m[m[:, 3] != 0]
    return M._pull(at, m[:, :3], m[:, 3], eps2)


def accel(lists, xyz, w_eff, G, eps2, targets, levmom=None, far=True):
    """fp64 acceleration of the bodies `targets`: the stencil as a direct sum over the listed bodies
    (far_monopole_model.accel, far=False), then -- far=True -- the members of the cell's set"""
    out = M.accel(lists, xyz, w_eff, G, eps2, targets, far=False)
    if not far:
        return out
    if levmom is None:
        levmom = level_moments(lists, xyz, w_eff, G)
    pos = np.asarray(xyz, np.float32).astype(np.float64)
    cell = np.full(len(pos), -1, np.int64)
    for c, l in enumerate(lists):
        cell[l] = c
    targets = np.asarray(targets, np.int64)
    for c in np.unique(cell[targets]):
        mine = np.nonzero(cell[targets] == c)[0]
        out[mine] += far_part(levmom, G, pos[targets[mine]], c, eps2)
    return out


def far_bodies(G):
    """mean size of the set over the cells of the box (information)"""
    return float(np.mean([len(interaction_set(c, G)) for c in range(G ** 3)]))
