"""The field of the quadrupole method (PSAMD_FLAG_FAR_PYRAMID | PSAMD_FLAG_FAR_QUADRUPOLE) at chosen points, restated in numpy
from include/psamd.h ("energy", "the field at chosen points", "quadrupoles on the pyramid") on far_model.py's pieces: what
PSAMD_POTENTIAL_FAR | PSAMD_POTENTIAL_QUADRUPOLE and PSAMD_PROBE_FAR | PSAMD_PROBE_QUADRUPOLE are held against
(test_far_quad_potential_cpu.py, test_gpu_far_quad_potential.py).  far_model.py's own phi64, phi32 and accel64 stop at the
pyramid's monopoles; the frames, the points, the moments and the order of every sum are as described there.

The potential's sums run over w * u and phi = -sum.  In that convention a far body (X, Y, Z, M != 0, C) adds its monopole term
M u and the quadrupole term
    t_q = 1.5 (d.C.d) u^5 - 0.5 T u^3,      d = (X, Y, Z) - x,  u = (d.d + eps2)^(-1/2),  T = Cxx + Cyy + Czz,
the term whose gradient is far_model.quad_pull's a_q."""
import numpy as np

import far_model as F
from far_model import _by_cell, _gather, _terms32

METHOD = "quadrupole"


def _matrices(cen):
    C = np.empty((len(cen), 3, 3))
    for f, (a, b) in enumerate(F.PLANES):
        C[:, a, b] = C[:, b, a] = cen[:, f]
    return C


def quad_terms64(at, bodies, cen, eps2):
    """fp64 [t, b]: t_q of every body at every point"""
    C = _matrices(np.asarray(cen, np.float64))
    d = bodies[None, :, :] - at[:, None, :]
    u = 1.0 / np.sqrt((d * d).sum(2) + eps2)
    dCd = (np.einsum("bij,tbj->tbi", C, d) * d).sum(2)
    T = np.trace(C, axis1=1, axis2=2)[None, :]
    return 1.5 * dCd * u ** 5 - 0.5 * T * u ** 3


def quad_sum64(lists, xyz, w_eff, G, eps2, at, cell, moments=None):
    """fp64 [t]: the sum of t_q over the far set's members (M != 0) of every point's cell -- phi's quadrupole part is minus this"""
    at = np.asarray(at, np.float32).astype(np.float64)
    if moments is None:
        moments = F.level_moments(lists, xyz, w_eff, G, METHOD)
    out = np.zeros(len(at))
    for _, mine, _, members in _by_cell(lists, G, cell, METHOD, moments, True):
        m = _gather(moments[0], members, 4)
        out[mine] = quad_terms64(at[mine], m[:, :3], _gather(moments[1], members, 6), eps2).sum(1)
    return out


def phi64(lists, xyz, w_eff, G, eps2, at, cell, own, moments=None):
    """fp64: the pyramid's phi over the same float32-rounded monopoles (far_model.phi64) minus the members' quadrupole terms"""
    if moments is None:
        moments = F.level_moments(lists, xyz, w_eff, G, METHOD)
    mono = F.phi64(lists, xyz, w_eff, G, eps2, at, cell, own, "pyramid", (moments[0], None))
    return mono - quad_sum64(lists, xyz, w_eff, G, eps2, at, cell, moments)


def accel64(lists, xyz, w_eff, G, eps2, at, cell, moments=None):
    """fp64 acceleration at probes (no own entry): the stencil's listed bodies, the members' monopoles, their quadrupole terms"""
    at = np.asarray(at, np.float32).astype(np.float64)
    return F._accel(lists, xyz, w_eff, G, eps2, at, cell, METHOD, moments, ("near", "mono", "quad"))


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


def _chain(t):
    """one fp32 chain from +0 in index order (add.accumulate is sequential), as an fp64 value per point"""
    return np.add.accumulate(t, axis=1, dtype=np.float32)[:, -1].astype(np.float64)


def phi32(lists, xyz, w_eff, G, eps2, at, cell, own, moments=None):
    """float32: the device's association.  The stencil's chains and every block's monopole chain are far_model.phi32's for the
    pyramid; behind a block's monopole chain comes that block's quadrupole chain -- one fp32 chain from +0, in index order, over
    the same members --, each carried into the fp64 sum by an addition of its own"""
    pos = np.asarray(xyz, np.float32)
    w = np.asarray(w_eff, np.float32)
    at = np.asarray(at, np.float32)
    own = np.asarray(own, np.int64)
    eps2f = np.float32(eps2)
    if moments is None:
        moments = F.level_moments(lists, xyz, w_eff, G, METHOD)
    out = np.zeros(len(at), np.float32)
    for c, mine, _, members in _by_cell(lists, G, cell, METHOD, moments, True):
        acc = np.zeros(len(mine))
        for k in F.stencil_cells(c, G):
            l = np.asarray(lists[k], np.int64)
            if len(l):
                t = _terms32(at[mine], pos[l], w[l], eps2f)
                t[l[None, :] == own[mine][:, None]] = np.float32(0.0)
                for j0 in range(0, t.shape[1], 64):
                    acc += _chain(t[:, j0:j0 + 64])
        for lvl, J in members:
            for b in np.unique(J >> 6):                                   # a block of 64 consecutive indices
                Jb = J[(J >> 6) == b]
                m = moments[0][lvl][Jb]
                acc += _chain(_terms32(at[mine], m[:, :3], m[:, 3], eps2f))
                acc += _chain(quad_terms32(at[mine], m[:, :3], moments[1][lvl][Jb], eps2f))
        out[mine] = (-acc).astype(np.float32)
    return out
