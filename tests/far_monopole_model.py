"""Far-field gravity from per-cell monopoles (PSAMD_FLAG_FAR_MONOPOLE), restated in numpy from the definition in
include/psamd.h -- not from the library's code.  Shared by test_far_monopole_cpu.py, test_gpu_far_monopole.py and
scripts/far_monopole_cost.py.

A frame is given as `lists` (per global cell, the indices of its listed bodies in list order), positions (float32 [n, 3])
and w_eff (float32 [n]: 0 for a kid, force_sign folded in).  Cells are numbered as the library numbers them:
c = (i3 * G + i1) * G + i2 with i2 ~ +x, i1 ~ -y, i3 ~ -z."""
import numpy as np


def cell_coords_of(xyz, G, cell_size=5.0):
    """(i1, i2, i3) of every position: floor((+-1.0 * c) / cell_size) + G // 2 in fp64"""
    p = np.asarray(xyz, np.float64)
    i2 = np.floor(p[:, 0] / cell_size).astype(np.int64) + G // 2
    i1 = np.floor(-p[:, 1] / cell_size).astype(np.int64) + G // 2
    i3 = np.floor(-p[:, 2] / cell_size).astype(np.int64) + G // 2
    return i1, i2, i3


def cells_of(xyz, G, cell_size=5.0):
    i1, i2, i3 = cell_coords_of(xyz, G, cell_size)
    assert min(i1.min(), i2.min(), i3.min()) >= 0 and max(i1.max(), i2.max(), i3.max()) < G, "a position outside the box"
    return (i3 * G + i1) * G + i2


def lists_of(xyz, G, cell_size=5.0, cap=None):
    """per cell the indices of its bodies, ascending (the library's lists are id-ascending), the first `cap` of them"""
    c = cells_of(xyz, G, cell_size)
    order = np.argsort(c, kind="stable")
    bounds = np.searchsorted(c[order], np.arange(G ** 3 + 1))
    return [order[bounds[k]:bounds[k + 1]][:cap] for k in range(G ** 3)]


def moments(lists, xyz, w_eff):
    """float32 [cells, 4] = (X, Y, Z, M): S = sum w_eff and sum w_eff * x, y, z in fp64, SEQUENTIALLY in list order (cumsum;
    np.sum adds pairwise), M = (float)S, X = (float)(Sx / S); S == 0: all four are 0"""
    xyz = np.asarray(xyz, np.float32)
    w_eff = np.asarray(w_eff, np.float32)
    out = np.zeros((len(lists), 4), np.float32)
    for c, l in enumerate(lists):
        if len(l) == 0:
            continue
        w = w_eff[l].astype(np.float64)
        S = np.cumsum(w)[-1]
        if S == 0.0:
            continue
        for k in range(3):
            out[c, k] = np.float32(np.cumsum(w * xyz[l, k].astype(np.float64))[-1] / S)
        out[c, 3] = np.float32(S)
    return out


def stencil_cells(c, G):
    """the cells of c's non-periodic 27-cell stencil"""
    i3, rem = divmod(int(c), G * G)
    i1, i2 = divmod(rem, G)
    return [(j3 * G + j1) * G + j2 for j3 in range(max(i3 - 1, 0), min(i3 + 2, G)) for j1 in range(max(i1 - 1, 0), min(i1 + 2, G))
            for j2 in range(max(i2 - 1, 0), min(i2 + 2, G))]


def _pull(at, bodies, mass, eps2):
    """fp64 acceleration at the points `at` [t, 3] from `bodies` [b, 3] with `mass` [b] (a body on the point adds nothing)"""
    d = bodies[None, :, :] - at[:, None, :]
    r2 = (d * d).sum(2) + eps2
    return (d * (mass / (r2 * np.sqrt(r2)))[:, :, None]).sum(1)


def accel(lists, xyz, w_eff, G, eps2, targets, mom=None, far=True):
    """fp64 acceleration of the bodies `targets` (indices; each must be in a list): the stencil as a direct sum over the
    listed bodies, then -- far=True -- one body per cell beyond the stencil from the float32-rounded moments `mom`
    (default: moments() of the frame); a cell with M == 0 adds nothing"""
    pos = np.asarray(xyz, np.float32).astype(np.float64)
    w = np.asarray(w_eff, np.float32).astype(np.float64)
    if far and mom is None:
        mom = moments(lists, xyz, w_eff)
    cell = np.full(len(pos), -1, np.int64)
    for c, l in enumerate(lists):
        cell[l] = c
    targets = np.asarray(targets, np.int64)
    assert (cell[targets] >= 0).all()
    out = np.zeros((len(targets), 3))
    for c in np.unique(cell[targets]):
        mine = np.nonzero(cell[targets] == c)[0]
        st = stencil_cells(c, G)
        near = np.concatenate([lists[k] for k in st]).astype(np.int64)
        a = _pull(pos[targets[mine]], pos[near], w[near], eps2)
        if far:
            rest = np.ones(len(lists), bool)
            rest[st] = False
            rest &= mom[:, 3] != 0
            m = mom[rest].astype(np.float64)
            a = a + _pull(pos[targets[mine]], m[:, :3], m[:, 3], eps2)
        out[mine] = a
    return out


def direct(xyz, w_eff, eps2, targets, chunk=64):
    """fp64 direct sum over ALL bodies"""
    pos = np.asarray(xyz, np.float32).astype(np.float64)
    w = np.asarray(w_eff, np.float32).astype(np.float64)
    targets = np.asarray(targets, np.int64)
    out = np.zeros((len(targets), 3))
    for k in range(0, len(targets), chunk):
        out[k:k + chunk] = _pull(pos[targets[k:k + chunk]], pos, w, eps2)
    return out


def rel_dev(got, want):
    return np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
