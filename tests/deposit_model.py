"""The mass on a lattice (psamd_deposit), written with numpy from include/psamd.h ("mass on a lattice") alone.

A frame is what psamd_build_grid leaves: the sorted snapshot x, y, z, w_eff (float32, by sorted index) and cell_start (the
exclusive prefix of the cells' counts: cell c lists the sorted indices cell_start[c] .. cell_start[c + 1], of which the first
min(count, cap) are bodies).  Cells and voxels are numbered as the library numbers them: cell (i3 G + i1) G + i2 with
(i1, i2, i3) along (-y, x, -z), voxel (n3 M + n1) M + n2.

deposit(...)        the definition: fp32 weights and terms, every operation a numpy float32 operation (rounded on its own),
                    the terms summed in fp64 (np.add.at: entry after entry) and rounded to float32 at the end
deposit(exact=True) the plain fp64 form for accuracy checks: exact weights from the positions, no fp32 anywhere; also the mass
                    within reach of every voxel ("support"), which the derived bound between the two forms is stated in
Both apply the list cap, the kid rule (w_eff = 0: a term of +0), the non-finite rule and the stencil rule."""
import math

import numpy as np

RESULT_KEYS = ("voxels", "bodies", "skipped", "mass", "vmax")
REFINES = (1, 2, 4)


def locate(x, y, z, G, cell_size):
    """Geometry::locate: the cell of float32 points, -1 outside the box"""
    x, y, z = (np.asarray(a, np.float32).astype(np.float64) for a in (x, y, z))
    with np.errstate(invalid="ignore"):
        d1, d2, d3 = np.floor(-y / cell_size) + G // 2, np.floor(x / cell_size) + G // 2, np.floor(-z / cell_size) + G // 2
        ok = (d1 >= 0) & (d1 < G) & (d2 >= 0) & (d2 < G) & (d3 >= 0) & (d3 < G)
    cell = np.full(len(x), -1, np.int64)
    cell[ok] = ((d3[ok] * G + d1[ok]) * G + d2[ok]).astype(np.int64)
    return cell


def frame_of(x, y, z, w_eff, cell, G):
    """a frame from particles and their cells as build_grid sorts them: cell-major, index ascending inside a cell.
    Returns (x, y, z, w_eff in sorted order, cell_start, the order)"""
    cell = np.asarray(cell, np.int64)
    order = np.argsort(cell, kind="stable")
    start = np.zeros(G ** 3 + 1, np.int64)
    np.cumsum(np.bincount(cell, minlength=G ** 3), out=start[1:])
    f = lambda a: np.asarray(a, np.float32)[order]
    return f(x), f(y), f(z), f(w_eff), start, order


def centres(G, cell_size, refine):
    """q_a of the voxel centres of one axis (float64 [M]): (n + 1/2 - (G / 2) k) h"""
    return (np.arange(G * refine) + 0.5 - (G // 2) * refine) * (cell_size / refine)


def _axis32(s, G, cell_size, k):
    inv_h = np.float32(np.float64(k) / np.float64(cell_size))
    off = np.float32((G // 2) * k) - np.float32(0.5)
    with np.errstate(over="ignore"):
        t = s * inv_h                                   # float32 array times float32 scalar: one fp32 rounding
        u = t + off
    uc = np.minimum(np.maximum(u, np.float32(0)), np.float32(G * k - 1))
    fl = np.floor(uc)
    f = uc - fl
    assert t.dtype == u.dtype == f.dtype == np.float32
    return fl.astype(np.int64), np.float32(1) - f, f


def _axis64(s, G, cell_size, k):
    u = s.astype(np.float64) * k / cell_size + ((G // 2) * k - 0.5)
    uc = np.minimum(np.maximum(u, 0.0), float(G * k - 1))
    fl = np.floor(uc)
    f = uc - fl
    return fl.astype(np.int64), 1.0 - f, f, u


def deposit(x, y, z, w_eff, cell_start, G, cell_size, cap, refine, exact=False, served=None):
    """{"rho": float32 [M, M, M] indexed [n3, n1, n2] (exact: float64), "sums": the fp64 sums before the rounding, "voxels",
    "bodies", "skipped", "mass" (fsum of the sums), "vmax"; exact: also "support", the mass of the bodies within one voxel
    (and u's rounding) of every voxel centre}.  served: a bool array by cell, the cells whose voxels are written and whose
    lists are counted (None: all)."""
    assert refine in REFINES
    k, M = refine, G * refine
    x, y, z, w_eff = (np.asarray(a, np.float32) for a in (x, y, z, w_eff))
    cell_start = np.asarray(cell_start, np.int64)
    ncell = G ** 3
    served = np.ones(ncell, bool) if served is None else np.asarray(served, bool)
    count = np.minimum(np.diff(cell_start)[:ncell], cap)                  # the list cap
    idx = np.concatenate([np.arange(cell_start[c], cell_start[c] + count[c]) for c in range(ncell)] or [np.zeros(0, np.int64)]).astype(np.int64)
    own = np.repeat(np.arange(ncell), count)                               # a body's cell is the list it is in
    bx, by, bz, bw = x[idx], y[idx], z[idx], w_eff[idx]
    fin = np.isfinite(bx) & np.isfinite(by) & np.isfinite(bz) & np.isfinite(bw)
    bodies, skipped = int((fin & served[own]).sum()), int((~fin & served[own]).sum())
    bx, by, bz, bw, own = bx[fin], by[fin], bz[fin], bw[fin], own[fin]
    m = np.abs(bw)                                                         # force_sign does not enter; a kid's is 0
    c3, r = np.divmod(own, G * G)
    c1, c2 = np.divmod(r, G)
    if exact:
        ax = [_axis64(s, G, cell_size, k) for s in (-by, bx, -bz)]
        m = m.astype(np.float64)
    else:
        ax = [_axis32(s, G, cell_size, k) for s in (-by, bx, -bz)]
    sums = np.zeros(M ** 3, np.float64)
    for d3 in (0, 1):
        for d1 in (0, 1):
            for d2 in (0, 1):
                n1, n2, n3 = ax[0][0] + d1, ax[1][0] + d2, ax[2][0] + d3
                W1, W2, W3 = ax[0][1 + d1], ax[1][1 + d2], ax[2][1 + d3]
                # a weight for n0 + 1 == M is dropped; the stencil rule: the voxel's cell within one cell of the body's
                ok = (n1 < M) & (n2 < M) & (n3 < M)
                ok &= (np.abs(n1 // k - c1) <= 1) & (np.abs(n2 // k - c2) <= 1) & (np.abs(n3 // k - c3) <= 1)
                term = ((W1 * W2) * W3) * m                                # fp32: three roundings more (exact: fp64)
                assert term.dtype == (np.float64 if exact else np.float32)
                np.add.at(sums, ((n3 * M + n1) * M + n2)[ok], term[ok].astype(np.float64))
    vox_cell = np.arange(M) // k
    vserved = served.reshape(G, G, G)[np.ix_(vox_cell, vox_cell, vox_cell)]        # [n3, n1, n2] <- cell [i3, i1, i2]
    sums = np.where(vserved, sums.reshape(M, M, M), 0.0)
    rho = sums if exact else sums.astype(np.float32)
    out = {"rho": rho, "sums": sums, "voxels": int(vserved.sum()), "bodies": bodies, "skipped": skipped,
           "mass": math.fsum(sums.ravel().tolist()), "vmax": float(rho[vserved].max()) if vserved.any() else -math.inf}
    if exact:
        # the mass within reach of a voxel: bodies with |u - n| < 1 on every axis, widened by u's fp32 rounding (M 2^-23)
        sup = np.zeros(M ** 3, np.float64)
        reach = 1.0 + M * 2.0 ** -23
        ucs = [np.minimum(np.maximum(a[3], 0.0), float(M - 1)) for a in ax]
        for o3 in (-1, 0, 1, 2):
            for o1 in (-1, 0, 1, 2):
                for o2 in (-1, 0, 1, 2):
                    n1, n2, n3 = ax[0][0] + o1, ax[1][0] + o2, ax[2][0] + o3
                    ok = (n1 >= 0) & (n1 < M) & (n2 >= 0) & (n2 < M) & (n3 >= 0) & (n3 < M)
                    ok &= (np.abs(ucs[0] - n1) < reach) & (np.abs(ucs[1] - n2) < reach) & (np.abs(ucs[2] - n3) < reach)
                    np.add.at(sup, ((n3 * M + n1) * M + n2)[ok], m[ok])
        out["support"] = sup.reshape(M, M, M)
    return out
