"""The far form of psamd_potential / psamd_probe (PSAMD_POTENTIAL_FAR, PSAMD_PROBE_FAR), restated in numpy from the
definition in include/psamd.h ("energy", far-monopole contexts) -- not from the library's code.  Lists, moments and sets are
far_monopole_model.py's and far_pyramid_model.py's, unchanged.  Shared by test_far_potential_cpu.py,
test_gpu_far_potential.py and scripts/far_potential_cost.py.

A frame is given as in far_monopole_model.py: `lists`, positions (float32 [n, 3]; a kid's TRUE position) and w_eff
(float32 [n]: 0 for a kid, force_sign folded in).  Points are given as positions `at` [t, 3], their cells `cell` [t] and
`own` [t]: the index of the body the point is (left out of its own cell's list by index), or -1 for a probe.

Two forms: phi64 is the method in fp64; phi32 is the device's association -- fp32 terms, fp32 chains of at most 64 from
+0 per stencil cell and per block of 64 level cells, carried on in fp64 -- with correctly rounded fp32 sqrt and division
where the device has the hardware reciprocal square root (ALLOW says what that may cost)."""
import numpy as np

import far_monopole_model as M
import far_pyramid_model as Y

# phi32 against the device, relative to |phi| when all terms have one sign.  A term: the hardware rsq is within 1 ulp of
# 1/sqrt (2^-23), the model's sqrt-then-divide within two half-ulps (2^-23), the product by M rounds once on either side
# (2^-23 between them): 3 * 2^-23 a term.  Terms that differ let every one of a chain's 64 additions round differently: 64 *
# 2^-24 = 2^-18 at the worst.  The last rounding to fp32: 2^-24.  (The fp64 carries differ by 1e-16: nothing.)
ALLOW = 2.0 ** -18 + 3 * 2.0 ** -23 + 2.0 ** -24


def levels(G, pyramid):
    return Y.levels_of(G) if pyramid else [int(G)]


def level_moments(lists, xyz, w_eff, G, pyramid):
    """per level float32 [G_l^3, 4] = (X, Y, Z, M); the flat method is one level"""
    return Y.level_moments(lists, xyz, w_eff, G) if pyramid else [M.moments(lists, xyz, w_eff)]


def far_set(c, G, pyramid):
    """[(level, level cell index)] in the order of the walk: levels top down, index order within a level"""
    if pyramid:
        return Y.interaction_set(c, G)
    near = set(M.stencil_cells(c, G))
    return [(0, J) for J in range(G ** 3) if J not in near]


def far_levels_of_set(c, G, pyramid):
    """far_set by level, top down: [(level, ascending level cell indices)]"""
    if not pyramid:
        keep = np.ones(G ** 3, bool)
        keep[M.stencil_cells(c, G)] = False
        return [(0, np.nonzero(keep)[0])]
    members = Y.interaction_set(c, G)
    return [(lvl, np.array([j for lv, j in members if lv == lvl], np.int64)) for lvl in range(len(Y.levels_of(G)) - 1, -1, -1)]


def _far_moments(levmom, c, G, pyramid):
    """float64 [b, 4]: the members with M != 0, in the order of the walk"""
    m = np.concatenate([levmom[lvl][J] for lvl, J in far_levels_of_set(c, G, pyramid)]).astype(np.float64).reshape(-1, 4)
    return m[m[:, 3] != 0]


def _points_by_cell(cell):
    cell = np.asarray(cell, np.int64)
    return [(int(c), np.nonzero(cell == c)[0]) for c in np.unique(cell)]


def phi64(lists, xyz, w_eff, G, eps2, at, cell, own, levmom=None, pyramid=False, far=True):
    """fp64: phi = -(sum over the stencil's listed bodies except `own`, then over the far set's members with M != 0) of
    w / sqrt(r.r + eps2), the moments float32-rounded as the device has them"""
    pos = np.asarray(xyz, np.float32).astype(np.float64)
    w = np.asarray(w_eff, np.float32).astype(np.float64)
    at = np.asarray(at, np.float32).astype(np.float64)
    own = np.asarray(own, np.int64)
    if far and levmom is None:
        levmom = level_moments(lists, xyz, w_eff, G, pyramid)
    out = np.zeros(len(at))
    for c, mine in _points_by_cell(cell):
        near = np.concatenate([lists[k] for k in M.stencil_cells(c, G)]).astype(np.int64)
        d = pos[near][None, :, :] - at[mine][:, None, :]
        t = w[near][None, :] / np.sqrt((d * d).sum(2) + eps2)
        t[near[None, :] == own[mine][:, None]] = 0.0
        s = t.sum(1)
        if far:
            m = _far_moments(levmom, c, G, pyramid)
            d = m[None, :, :3] - at[mine][:, None, :]
            s = s + (m[None, :, 3] / np.sqrt((d * d).sum(2) + eps2)).sum(1)
        out[mine] = -s
    return out


def _terms32(at, bodies, mass, eps2f):
    """float32 [t, b]: fp32 differences, unfused r.r, + eps2, 1 / sqrt, one multiply by the mass"""
    r = bodies[None, :, :] - at[:, None, :]
    d2 = r[:, :, 0] * r[:, :, 0] + r[:, :, 1] * r[:, :, 1] + r[:, :, 2] * r[:, :, 2]
    return mass[None, :] * (np.float32(1.0) / np.sqrt(d2 + eps2f))


def _chains(acc, t):
    """the terms t [points, bodies] in fp32 chains of at most 64 from +0 (add.accumulate is sequential), carried in fp64"""
    for j0 in range(0, t.shape[1], 64):
        acc += np.add.accumulate(t[:, j0:j0 + 64], axis=1, dtype=np.float32)[:, -1].astype(np.float64)


def phi32(lists, xyz, w_eff, G, eps2, at, cell, own, levmom=None, pyramid=False, far=True):
    """float32: the device's association.  The stencil's cells are taken in index order, not the reference's: a cell's
    chains do not depend on it, only the order of the fp64 carries does"""
    pos = np.asarray(xyz, np.float32)
    w = np.asarray(w_eff, np.float32)
    at = np.asarray(at, np.float32)
    own = np.asarray(own, np.int64)
    eps2f = np.float32(eps2)
    if far and levmom is None:
        levmom = level_moments(lists, xyz, w_eff, G, pyramid)
    out = np.zeros(len(at), np.float32)
    for c, mine in _points_by_cell(cell):
        acc = np.zeros(len(mine))
        for k in M.stencil_cells(c, G):
            l = np.asarray(lists[k], np.int64)
            if len(l):
                t = _terms32(at[mine], pos[l], w[l], eps2f)
                t[l[None, :] == own[mine][:, None]] = np.float32(0.0)
                _chains(acc, t)
        if far:
            for lvl, J in far_levels_of_set(c, G, pyramid):
                J = J[levmom[lvl][J, 3] != 0]
                for b in np.unique(J >> 6):                               # a block of 64 consecutive indices: one chain
                    m = levmom[lvl][J[(J >> 6) == b]]
                    acc += np.add.accumulate(_terms32(at[mine], m[:, :3], m[:, 3], eps2f), axis=1, dtype=np.float32)[:, -1].astype(np.float64)
        out[mine] = (-acc).astype(np.float32)
    return out


def direct_phi(xyz, w_eff, eps2, targets, chunk=64):
    """fp64 direct sum over ALL bodies but the target itself"""
    pos = np.asarray(xyz, np.float32).astype(np.float64)
    w = np.asarray(w_eff, np.float32).astype(np.float64)
    targets = np.asarray(targets, np.int64)
    out = np.zeros(len(targets))
    for k in range(0, len(targets), chunk):
        tk = targets[k:k + chunk]
        d = pos[None, :, :] - pos[tk][:, None, :]
        t = w[None, :] / np.sqrt((d * d).sum(2) + eps2)
        t[np.arange(len(tk)), tk] = 0.0
        out[k:k + chunk] = -t.sum(1)
    return out


def energy(w_eff, phi):
    """U = 1/2 sum |w_i| phi_i in fp64 over the finite ones"""
    phi = np.asarray(phi, np.float64)
    ok = np.isfinite(phi)
    return 0.5 * float((np.abs(np.asarray(w_eff, np.float64))[ok] * phi[ok]).sum())


def accel64(lists, xyz, w_eff, G, eps2, at, cell, levmom=None, pyramid=False):
    """fp64 acceleration at probes (no own entry): the stencil's listed bodies, then the far set's members"""
    pos = np.asarray(xyz, np.float32).astype(np.float64)
    w = np.asarray(w_eff, np.float32).astype(np.float64)
    at = np.asarray(at, np.float32).astype(np.float64)
    if levmom is None:
        levmom = level_moments(lists, xyz, w_eff, G, pyramid)
    out = np.zeros((len(at), 3))
    for c, mine in _points_by_cell(cell):
        near = np.concatenate([lists[k] for k in M.stencil_cells(c, G)]).astype(np.int64)
        a = M._pull(at[mine], pos[near], w[near], eps2)
        m = _far_moments(levmom, c, G, pyramid)
        out[mine] = a + M._pull(at[mine], m[:, :3], m[:, 3], eps2)
    return out
