"""Quadrupoles on the pyramid (PSAMD_FLAG_FAR_QUADRUPOLE), restated in numpy from the definition in include/psamd.h
("quadrupoles on the pyramid") on top of far_pyramid_model.py -- not from the library's code.  Shared by
test_far_quadrupole_cpu.py, test_gpu_far_quadrupole.py and scripts/far_quadrupole_cost.py.

Frames, lists, levels and the interaction set are far_pyramid_model.py's.  The planes of second moments go in the order
xx, yy, zz, xy, xz, yz."""
import numpy as np

import far_monopole_model as M
import far_pyramid_model as Y

PLANES = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def level_sums(lists, xyz, w_eff, G):
    """per level float64 [G_l^3, 10] = (S, Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz).  Level 0: sequentially in list order, the
    term of an entry RN(RN(w * x_a) * x_b) (w * x_a is exact in fp64).  Level l + 1: the children's sums added one at a time
    in ascending child index to +0, as far_pyramid_model.level_sums does its four"""
    xyz = np.asarray(xyz, np.float32)
    w_eff = np.asarray(w_eff, np.float32)
    dims = Y.levels_of(G)
    s0 = np.zeros((G ** 3, 10))
    for c, l in enumerate(lists):
        if len(l):
            w = w_eff[l].astype(np.float64)
            x = xyz[l].astype(np.float64)
            s0[c, 0] = np.cumsum(w)[-1]
            for k in range(3):
                s0[c, 1 + k] = np.cumsum(w * x[:, k])[-1]
            for f, (a, b) in enumerate(PLANES):
                s0[c, 4 + f] = np.cumsum((w * x[:, a]) * x[:, b])[-1]
    out = [s0]
    for lvl in range(1, len(dims)):
        Gc, Gp = dims[lvl - 1], dims[lvl]
        child = np.zeros((2 * Gp, 2 * Gp, 2 * Gp, 10))               # [k3, k1, k2]
        child[:Gc, :Gc, :Gc] = out[-1].reshape(Gc, Gc, Gc, 10)
        acc = np.zeros((Gp, Gp, Gp, 10))
        for d3 in (0, 1):                                            # ascending child index: k3 slowest, k2 fastest
            for d1 in (0, 1):
                for d2 in (0, 1):
                    acc = acc + child[d3::2, d1::2, d2::2]
        out.append(acc.reshape(Gp ** 3, 10))
    return out


def central_of(s):
    """float32 [cells, 6] from one level's sums: C_ab = (float)(S_ab - RN(RN(S_a / S) * S_b)); S == 0: six zeros"""
    c = np.zeros((len(s), 6), np.float32)
    nz = s[:, 0] != 0.0
    for f, (a, b) in enumerate(PLANES):
        c[nz, f] = (s[nz, 4 + f] - (s[nz, 1 + a] / s[nz, 0]) * s[nz, 1 + b]).astype(np.float32)
    return c


def level_moments(lists, xyz, w_eff, G):
    """(per level float32 [G_l^3, 4] = (X, Y, Z, M) -- far_pyramid_model.level_moments' bits --, per level float32 [G_l^3, 6] =
    the central second moments)"""
    mom, cen = [], []
    for s in level_sums(lists, xyz, w_eff, G):
        m = np.zeros((len(s), 4), np.float32)
        nz = s[:, 0] != 0.0
        m[nz, :3] = (s[nz, 1:4] / s[nz, :1]).astype(np.float32)
        m[nz, 3] = s[nz, 0].astype(np.float32)
        mom.append(m)
        cen.append(central_of(s))
    return mom, cen


def quad_pull(at, bodies, cen, eps2):
    """fp64 quadrupole acceleration at the points `at` [t, 3] from `bodies` [b, 3] with the central moments `cen` [b, 6]:
    a_q = -3 (C d) u^5 + 7.5 (d.C.d) u^7 d - 1.5 T u^5 d, d = body - point, u = (d.d + eps2)^(-1/2), T = Cxx + Cyy + Czz"""
    C = np.empty((len(bodies), 3, 3))
    for f, (a, b) in enumerate(PLANES):
        C[:, a, b] = C[:, b, a] = cen[:, f]
    d = bodies[None, :, :] - at[:, None, :]
    u = 1.0 / np.sqrt((d * d).sum(2) + eps2)
    Cd = np.einsum("bij,tbj->tbi", C, d)
    dCd = (Cd * d).sum(2)
    T = np.trace(C, axis1=1, axis2=2)[None, :]
    u5, u7 = u ** 5, u ** 7
    return (-3.0 * Cd * u5[:, :, None] + ((7.5 * dCd * u7 - 1.5 * T * u5)[:, :, None]) * d).sum(1)


def quad_part(levmom, levcen, G, at, c, eps2):
    """fp64 quadrupole acceleration at the points `at` [t, 3], all of cell c, from the members of c's set (M != 0) with the
    float32-rounded moments of level_moments()"""
    members = Y.interaction_set(c, G)
    m = np.array([levmom[lvl][J] for lvl, J in members], np.float64).reshape(-1, 4)
    q = np.array([levcen[lvl][J] for lvl, J in members], np.float64).reshape(-1, 6)
    keep = m[:, 3] != 0
    return quad_pull(at, m[keep, :3], q[keep], eps2)


def quad_accel(lists, xyz, w_eff, G, eps2, targets, moments=None):
    """fp64 quadrupole part of the acceleration of the bodies `targets`"""
    levmom, levcen = level_moments(lists, xyz, w_eff, G) if moments is None else moments
    pos = np.asarray(xyz, np.float32).astype(np.float64)
    cell = np.full(len(pos), -1, np.int64)
    for c, l in enumerate(lists):
        cell[l] = c
    targets = np.asarray(targets, np.int64)
    assert (cell[targets] >= 0).all()
    out = np.zeros((len(targets), 3))
    for c in np.unique(cell[targets]):
        mine = np.nonzero(cell[targets] == c)[0]
        out[mine] = quad_part(levmom, levcen, G, pos[targets[mine]], c, eps2)
    return out


def accel(lists, xyz, w_eff, G, eps2, targets, moments=None):
    """fp64 acceleration of the bodies `targets`: the pyramid model's (stencil + monopoles of the set) + the quadrupole part"""
    if moments is None:
        moments = level_moments(lists, xyz, w_eff, G)
    return Y.accel(lists, xyz, w_eff, G, eps2, targets, levmom=moments[0]) + quad_accel(lists, xyz, w_eff, G, eps2, targets, moments)
