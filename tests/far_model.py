"""The far field restated in numpy from the definitions in include/psamd.h ("long-range gravity", "a pyramid of monopoles",
"quadrupoles on the pyramid", "energy", "the field at chosen points") -- not from the library's code.  Shared by the
test_far_*_cpu.py suites, far_force_suite.py, far_field_suite.py and scripts/far_*.py; tests/golden/far_model.json and
tests/golden/far_field_quadrupole.json pin what it computes (scripts/far_model_golden.py).

A METHOD is one of
    flat         PSAMD_FLAG_FAR_MONOPOLE: one monopole per cell beyond the stencil -- a pyramid of one level
    pyramid      PSAMD_FLAG_FAR_PYRAMID: coarser monopoles for farther mass
    quadrupole   PSAMD_FLAG_FAR_PYRAMID | PSAMD_FLAG_FAR_QUADRUPOLE: the pyramid's monopoles and the quadrupole term of each
and everything below takes the method as an argument.

A frame is given as `lists` (per global cell, the indices of its listed bodies in list order), positions (float32 [n, 3]; a
kid's TRUE position) and w_eff (float32 [n]: 0 for a kid, force_sign folded in).  Cells are numbered as the library numbers
them: c = (i3 * G + i1) * G + i2 with i2 ~ +x, i1 ~ -y, i3 ~ -z; a level-l cell is numbered (k3 * G_l + k1) * G_l + k2.  The planes
of second moments go in the order xx, yy, zz, xy, xz, yz.  Points are given as positions `at` [t, 3], their cells `cell` [t] and
`own` [t]: the index of the body the point is (left out of its own cell's list by index), or -1 for a probe.

The order of bodies in every sum is part of what the model states: stencil cells in index order, far members in the order of
the walk (levels top down, index order within a level), cumsum for the sequential sums (np.sum adds pairwise).

Two forms of the potential: phi64 is the method in fp64; phi32 is the device's association -- fp32 terms, fp32 chains of at most
64 from +0 per stencil cell and per block of 64 level cells, carried on in fp64 -- with correctly rounded fp32 sqrt and division
where the device has the hardware reciprocal square root (ALLOW says what that may cost).

The potential's sums run over w * u and phi = -sum.  In that convention a far body (X, Y, Z, M != 0, C) of the quadrupole method
adds its monopole term M u and the quadrupole term
    t_q = 1.5 (d.C.d) u^5 - 0.5 T u^3,      d = (X, Y, Z) - x,  u = (d.d + eps2)^(-1/2),  T = Cxx + Cyy + Czz,
the term whose gradient is quad_pull's a_q."""
import numpy as np

METHODS = ("flat", "pyramid", "quadrupole")
PLANES = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))

# phi32 against the device, relative to |phi| when all terms have one sign.  A term: the hardware rsq is within 1 ulp of
# 1/sqrt (2^-23), the model's sqrt-then-divide within two half-ulps (2^-23), the product by M rounds once on either side
# (2^-23 between them): 3 * 2^-23 a term.  Terms that differ let every one of a chain's 64 additions round differently: 64 *
# 2^-24 = 2^-18 at the worst.  The last rounding to fp32: 2^-24.  (The fp64 carries differ by 1e-16: nothing.)
ALLOW = 2.0 ** -18 + 3 * 2.0 ** -23 + 2.0 ** -24


# ---- geometry ---------------------------------------------------------------------------------------------------------------

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


def stencil_cells(c, G):
    """the cells of c's non-periodic 27-cell stencil"""
    i3, rem = divmod(int(c), G * G)
    i1, i2 = divmod(rem, G)
    return [(j3 * G + j1) * G + j2 for j3 in range(max(i3 - 1, 0), min(i3 + 2, G)) for j1 in range(max(i1 - 1, 0), min(i1 + 2, G))
            for j2 in range(max(i2 - 1, 0), min(i2 + 2, G))]


def coords(c, G):
    i3, rem = divmod(int(c), G * G)
    i1, i2 = divmod(rem, G)
    return i1, i2, i3


def levels_of(G):
    """[G_0 .. G_L]: halved (rounded up) until at most 4"""
    dims = [int(G)]
    while dims[-1] > 4:
        dims.append((dims[-1] + 1) // 2)
    return dims


def levels(G, method):
    """the flat method is one level"""
    assert method in METHODS, method
    return [int(G)] if method == "flat" else levels_of(G)


def far_set_by_level(c, G, method):
    """the far set of a particle in cell c, by level, top down: [(level, ascending level cell indices)].  At the top level every
    cell not within 1 (max-norm) of c's; below it every cell whose parent is within 1 of c's parent and which is not itself
    within 1 of c's cell of that level.  (Flat: the top level is level 0, so every cell beyond the stencil.)"""
    dims = levels(G, method)
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
        out.append((lvl, ((j3 * Gl + j1) * Gl + j2)[far].astype(np.int64)))
    return out


def far_set(c, G, method):
    """[(level, level cell index)] in the order of the walk: levels top down, index order within a level"""
    return [(lvl, int(J)) for lvl, members in far_set_by_level(c, G, method) for J in members]


def coverage(c, G, method, members=None):
    """int [G^3]: how often every cell of the box is covered -- by c's stencil, or by a member of c's set (as a leaf under it)"""
    n = np.zeros(G ** 3, np.int64)
    n[stencil_cells(c, G)] += 1
    cube = n.reshape(G, G, G)                                         # [i3, i1, i2]; i >> lvl == j: i in [j << lvl, (j + 1) << lvl)
    dims = levels(G, method)
    members = far_set(c, G, method) if members is None else members
    for lvl, Gl in enumerate(dims):                                   # a level at a time: its members counted on the level's own cube,
        J = np.array([j for l, j in members if l == lvl], np.int64)      # every level cell then spread over the cells under it
        if len(J):
            level = np.bincount(J, minlength=Gl ** 3).reshape(Gl, Gl, Gl)
            for axis in range(3):
                level = np.repeat(level, 1 << lvl, axis=axis)
            cube += level[:G, :G, :G]
    return n


# ---- sums and moments ---------------------------------------------------------------------------------------------------------

def level_sums(lists, xyz, w_eff, G, method):
    """per level float64 [G_l^3, 4] = (S, Sx, Sy, Sz); `quadrupole`: [G_l^3, 10], then Sxx, Syy, Szz, Sxy, Sxz, Syz.  Every column is
    computed on its own, so the first four have the same bits under every method.  Level 0: sequentially in list order, the
    term of a second moment RN(RN(w * x_a) * x_b) (w * x_a is exact in fp64).  Level l + 1: the existing children's sums added
    one at a time in ascending child index to +0 -- a child that does not exist is entered as +0 here, which leaves every bit
    as it is"""
    xyz = np.asarray(xyz, np.float32)
    w_eff = np.asarray(w_eff, np.float32)
    dims = levels(G, method)
    cols = 10 if method == "quadrupole" else 4
    s0 = np.zeros((G ** 3, cols))
    for c, l in enumerate(lists):
        if len(l):
            w = w_eff[l].astype(np.float64)
            x = xyz[l].astype(np.float64)
            s0[c, 0] = np.cumsum(w)[-1]
            for k in range(3):
                s0[c, 1 + k] = np.cumsum(w * x[:, k])[-1]
            for f, (a, b) in enumerate(PLANES[:cols - 4]):
                s0[c, 4 + f] = np.cumsum((w * x[:, a]) * x[:, b])[-1]
    out = [s0]
    for lvl in range(1, len(dims)):
        Gc, Gp = dims[lvl - 1], dims[lvl]
        child = np.zeros((2 * Gp, 2 * Gp, 2 * Gp, cols))              # [k3, k1, k2]
        child[:Gc, :Gc, :Gc] = out[-1].reshape(Gc, Gc, Gc, cols)
        acc = np.zeros((Gp, Gp, Gp, cols))
        for d3 in (0, 1):                                            # ascending child index: k3 slowest, k2 fastest
            for d1 in (0, 1):
                for d2 in (0, 1):
                    acc = acc + child[d3::2, d1::2, d2::2]
        out.append(acc.reshape(Gp ** 3, cols))
    return out


def central_of(s):
    """float32 [cells, 6] from one level's sums: C_ab = (float)(S_ab - RN(RN(S_a / S) * S_b)); S == 0: six zeros"""
    c = np.zeros((len(s), 6), np.float32)
    nz = s[:, 0] != 0.0
    for f, (a, b) in enumerate(PLANES):
        c[nz, f] = (s[nz, 4 + f] - (s[nz, 1 + a] / s[nz, 0]) * s[nz, 1 + b]).astype(np.float32)
    return c


def level_moments(lists, xyz, w_eff, G, method):
    """(mom, cen): per level float32 [G_l^3, 4] = (X, Y, Z, M) with M = (float)S, X = (float)(Sx / S), S == 0: four zeros -- the same
    bits under every method --; and per level float32 [G_l^3, 6] = the central second moments, or None where the method has none"""
    sums = level_sums(lists, xyz, w_eff, G, method)
    mom = []
    for s in sums:
        m = np.zeros((len(s), 4), np.float32)
        nz = s[:, 0] != 0.0
        m[nz, :3] = (s[nz, 1:4] / s[nz, :1]).astype(np.float32)
        m[nz, 3] = s[nz, 0].astype(np.float32)
        mom.append(m)
    return mom, [central_of(s) for s in sums] if method == "quadrupole" else None


# ---- fields -------------------------------------------------------------------------------------------------------------------

def _pull(at, bodies, mass, eps2):
    """fp64 acceleration at the points `at` [t, 3] from `bodies` [b, 3] with `mass` [b] (a body on the point adds nothing)"""
    d = bodies[None, :, :] - at[:, None, :]
    r2 = (d * d).sum(2) + eps2
    return (d * (mass / (r2 * np.sqrt(r2)))[:, :, None]).sum(1)


def _matrices(cen):
    """float64 [b, 3, 3]: the symmetric matrices of the six planes `cen` [b, 6]"""
    C = np.empty((len(cen), 3, 3))
    for f, (a, b) in enumerate(PLANES):
        C[:, a, b] = C[:, b, a] = cen[:, f]
    return C


def quad_pull(at, bodies, cen, eps2):
    """fp64 quadrupole acceleration at the points `at` [t, 3] from `bodies` [b, 3] with the central moments `cen` [b, 6]:
    a_q = -3 (C d) u^5 + 7.5 (d.C.d) u^7 d - 1.5 T u^5 d, d = body - point, u = (d.d + eps2)^(-1/2), T = Cxx + Cyy + Czz"""
    C = _matrices(cen)
    d = bodies[None, :, :] - at[:, None, :]
    u = 1.0 / np.sqrt((d * d).sum(2) + eps2)
    Cd = np.einsum("bij,tbj->tbi", C, d)
    dCd = (Cd * d).sum(2)
    T = np.trace(C, axis1=1, axis2=2)[None, :]
    u5, u7 = u ** 5, u ** 7
    return (-3.0 * Cd * u5[:, :, None] + ((7.5 * dCd * u7 - 1.5 * T * u5)[:, :, None]) * d).sum(1)


def quad_terms64(at, bodies, cen, eps2):
    """fp64 [t, b]: t_q of every body at every point"""
    C = _matrices(np.asarray(cen, np.float64))
    d = bodies[None, :, :] - at[:, None, :]
    u = 1.0 / np.sqrt((d * d).sum(2) + eps2)
    dCd = (np.einsum("bij,tbj->tbi", C, d) * d).sum(2)
    T = np.trace(C, axis1=1, axis2=2)[None, :]
    return 1.5 * dCd * u ** 5 - 0.5 * T * u ** 3


def _by_cell(lists, G, cell, method, moments, far):
    """the one loop over the points' cells: (cell, its points, the stencil's listed bodies in index order of the cells, the far
    set by level with the members of M == 0 taken out -- [] without far)"""
    cell = np.asarray(cell, np.int64)
    for c in np.unique(cell):
        near = np.concatenate([lists[k] for k in stencil_cells(c, G)]).astype(np.int64)
        members = [(lvl, J[moments[0][lvl][J, 3] != 0]) for lvl, J in far_set_by_level(c, G, method)] if far else []
        yield int(c), np.nonzero(cell == c)[0], near, members


def _gather(planes, members, width):
    """float64 [b, width]: the members' rows of the levels' `planes`, in the order of the walk"""
    return np.concatenate([planes[lvl][J] for lvl, J in members]).astype(np.float64).reshape(-1, width)


def _accel(lists, xyz, w_eff, G, eps2, at, cell, method, moments, parts):
    """fp64, per point the sum of `parts` in this order: "near" (the stencil as a direct sum over the listed bodies), "mono" (the
    members' monopoles), "quad" (their quadrupole terms)"""
    pos = np.asarray(xyz, np.float32).astype(np.float64)
    w = np.asarray(w_eff, np.float32).astype(np.float64)
    far = parts != ("near",)
    if far and moments is None:
        moments = level_moments(lists, xyz, w_eff, G, method)
    out = np.zeros((len(at), 3))
    for c, mine, near, members in _by_cell(lists, G, cell, method, moments, far):
        terms = []
        if "near" in parts:
            terms.append(_pull(at[mine], pos[near], w[near], eps2))
        if far:
            m = _gather(moments[0], members, 4)
        if "mono" in parts:
            terms.append(_pull(at[mine], m[:, :3], m[:, 3], eps2))
        if "quad" in parts:
            terms.append(quad_pull(at[mine], m[:, :3], _gather(moments[1], members, 6), eps2))
        a = terms[0]
        for t in terms[1:]:
            a = a + t
        out[mine] = a
    return out


def _bodies(lists, xyz, targets):
    """(fp64 positions of the bodies `targets`, their cells); each must be in a list"""
    cell = np.full(len(xyz), -1, np.int64)
    for c, l in enumerate(lists):
        cell[l] = c
    targets = np.asarray(targets, np.int64)
    assert (cell[targets] >= 0).all()
    return np.asarray(xyz, np.float32).astype(np.float64)[targets], cell[targets]


def accel(lists, xyz, w_eff, G, eps2, targets, method, moments=None, far=True):
    """fp64 acceleration of the bodies `targets` (indices; each must be in a list): the stencil as a direct sum over the listed
    bodies, then -- far=True -- the monopoles of the far set's members from the float32-rounded `moments` (default:
    level_moments() of the frame; a member with M == 0 adds nothing), then the quadrupole part where the method has one"""
    assert method in METHODS, method
    at, cell = _bodies(lists, xyz, targets)
    parts = ("near",) if not far else ("near", "mono", "quad") if method == "quadrupole" else ("near", "mono")
    return _accel(lists, xyz, w_eff, G, eps2, at, cell, method, moments, parts)


def quad_accel(lists, xyz, w_eff, G, eps2, targets, moments=None):
    """fp64 quadrupole part of the acceleration of the bodies `targets`"""
    at, cell = _bodies(lists, xyz, targets)
    return _accel(lists, xyz, w_eff, G, eps2, at, cell, "quadrupole", moments, ("quad",))


def accel64(lists, xyz, w_eff, G, eps2, at, cell, method, moments=None):
    """fp64 acceleration at probes (no own entry): the stencil's listed bodies, the far set's monopoles, then their quadrupole
    terms where the method has them"""
    assert method in METHODS, method
    at = np.asarray(at, np.float32).astype(np.float64)
    return _accel(lists, xyz, w_eff, G, eps2, at, cell, method, moments, ("near", "mono", "quad") if method == "quadrupole" else ("near", "mono"))


def quad_sum64(lists, xyz, w_eff, G, eps2, at, cell, moments=None):
    """fp64 [t]: the sum of t_q over the far set's members (M != 0) of every point's cell -- phi's quadrupole part is minus this"""
    at = np.asarray(at, np.float32).astype(np.float64)
    if moments is None:
        moments = level_moments(lists, xyz, w_eff, G, "quadrupole")
    out = np.zeros(len(at))
    for _, mine, _, members in _by_cell(lists, G, cell, "quadrupole", moments, True):
        m = _gather(moments[0], members, 4)
        out[mine] = quad_terms64(at[mine], m[:, :3], _gather(moments[1], members, 6), eps2).sum(1)
    return out


def phi64(lists, xyz, w_eff, G, eps2, at, cell, own, method, moments=None, far=True):
    """fp64: phi = -(sum over the stencil's listed bodies except `own`, then over the far set's members with M != 0) of
    w / sqrt(r.r + eps2), the moments float32-rounded as the device has them; quadrupole: minus the members' quadrupole terms"""
    assert method in METHODS, method
    pos = np.asarray(xyz, np.float32).astype(np.float64)
    w = np.asarray(w_eff, np.float32).astype(np.float64)
    at = np.asarray(at, np.float32).astype(np.float64)
    own = np.asarray(own, np.int64)
    if far and moments is None:
        moments = level_moments(lists, xyz, w_eff, G, method)
    out = np.zeros(len(at))
    for c, mine, near, members in _by_cell(lists, G, cell, method, moments, far):
        d = pos[near][None, :, :] - at[mine][:, None, :]
        t = w[near][None, :] / np.sqrt((d * d).sum(2) + eps2)
        t[near[None, :] == own[mine][:, None]] = 0.0
        s = t.sum(1)
        if far:
            m = _gather(moments[0], members, 4)
            d = m[None, :, :3] - at[mine][:, None, :]
            s = s + (m[None, :, 3] / np.sqrt((d * d).sum(2) + eps2)).sum(1)
        out[mine] = -s
        if far and method == "quadrupole":
            out[mine] -= quad_terms64(at[mine], m[:, :3], _gather(moments[1], members, 6), eps2).sum(1)
    return out


def _terms32(at, bodies, mass, eps2f):
    """float32 [t, b]: fp32 differences, unfused r.r, + eps2, 1 / sqrt, one multiply by the mass"""
    r = bodies[None, :, :] - at[:, None, :]
    d2 = r[:, :, 0] * r[:, :, 0] + r[:, :, 1] * r[:, :, 1] + r[:, :, 2] * r[:, :, 2]
    return mass[None, :] * (np.float32(1.0) / np.sqrt(d2 + eps2f))


def _fma(a, b, c):
    """float32 fma(a, b, c): the product of two fp32 values is exact in fp64; the sum is rounded in fp64 and then to fp32 (a
    double rounding, which differs from one rounding in rare last bits: the model is held to a tolerance, not to bits)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def quad_terms32(at, bodies, cen, eps2f):
    """float32 [t, b]: the header's fp32 operation sequence for t_q, with a correctly rounded 1 / sqrt where the device has the
    hardware reciprocal square root"""
    f32 = np.float32
    at, bodies, cen = np.asarray(at, f32), np.asarray(bodies, f32), np.asarray(cen, f32)
    d = bodies[None, :, :] - at[:, None, :]
    dx, dy, dz = d[:, :, 0], d[:, :, 1], d[:, :, 2]
    r2 = (dx * dx + dy * dy) + dz * dz
    u = f32(1.0) / np.sqrt(r2 + f32(eps2f))
    u2 = u * u
    u3 = u2 * u
    u5 = u3 * u2
    cxx, cyy, czz, cxy, cxz, cyz = (np.broadcast_to(cen[None, :, k], dx.shape) for k in range(6))
    gx = _fma(cxz, dz, _fma(cxy, dy, cxx * dx))
    gy = _fma(cyz, dz, _fma(cyy, dy, cxy * dx))
    gz = _fma(czz, dz, _fma(cyz, dy, cxz * dx))
    q = _fma(gz, dz, _fma(gy, dy, gx * dx))
    T = (cxx + cyy) + czz
    t = _fma(f32(1.5) * u5, q, (f32(-0.5) * T) * u3)
    assert t.dtype == f32
    return t


def _chains(acc, t):
    """the terms t [points, bodies] in fp32 chains of at most 64 from +0 (add.accumulate is sequential), carried in fp64"""
    for j0 in range(0, t.shape[1], 64):
        acc += np.add.accumulate(t[:, j0:j0 + 64], axis=1, dtype=np.float32)[:, -1].astype(np.float64)


def phi32(lists, xyz, w_eff, G, eps2, at, cell, own, method, moments=None, far=True):
    """float32: the device's association.  The stencil's cells are taken in index order, not the reference's: a cell's
    chains do not depend on it, only the order of the fp64 carries does.  Quadrupole: behind a block's monopole chain comes that
    block's quadrupole chain -- one fp32 chain from +0, in index order, over the same members --, each carried into the fp64 sum
    by an addition of its own"""
    assert method in METHODS, method
    pos = np.asarray(xyz, np.float32)
    w = np.asarray(w_eff, np.float32)
    at = np.asarray(at, np.float32)
    own = np.asarray(own, np.int64)
    eps2f = np.float32(eps2)
    if far and moments is None:
        moments = level_moments(lists, xyz, w_eff, G, method)
    out = np.zeros(len(at), np.float32)
    for c, mine, _, members in _by_cell(lists, G, cell, method, moments, far):
        acc = np.zeros(len(mine))
        for k in stencil_cells(c, G):
            l = np.asarray(lists[k], np.int64)
            if len(l):
                t = _terms32(at[mine], pos[l], w[l], eps2f)
                t[l[None, :] == own[mine][:, None]] = np.float32(0.0)
                _chains(acc, t)
        for lvl, J in members:
            for b in np.unique(J >> 6):                                   # a block of 64 consecutive indices: one chain
                Jb = J[(J >> 6) == b]
                m = moments[0][lvl][Jb]
                _chains(acc, _terms32(at[mine], m[:, :3], m[:, 3], eps2f))
                if method == "quadrupole":
                    _chains(acc, quad_terms32(at[mine], m[:, :3], moments[1][lvl][Jb], eps2f))
        out[mine] = (-acc).astype(np.float32)
    return out


# ---- the direct sums they are held against ---------------------------------------------------------------------------------------

def direct(xyz, w_eff, eps2, targets, chunk=64):
    """fp64 direct sum over ALL bodies"""
    pos = np.asarray(xyz, np.float32).astype(np.float64)
    w = np.asarray(w_eff, np.float32).astype(np.float64)
    targets = np.asarray(targets, np.int64)
    out = np.zeros((len(targets), 3))
    for k in range(0, len(targets), chunk):
        out[k:k + chunk] = _pull(pos[targets[k:k + chunk]], pos, w, eps2)
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


def rel_dev(got, want):
    return np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
