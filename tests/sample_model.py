"""A lattice field at points (psamd_sample), written with numpy from include/psamd.h ("a lattice field at the particles") alone.

The lattice, the axes and the weights are psamd_deposit's (deposit_model: locate, _axis32); a field is a float32 array
[M, M, M] or [M, M, M, 4] indexed [n3, n1, n2].  Every fp32 operation is a numpy float32 operation (rounded on its own); the
eight terms of an entry go into one float64 chain per component in the order (d3, d1, d2), each 0 then 1, by a Python loop --
not np.sum, whose order is its own.

sample(...)      (out, outcomes, the result record as a dict, S) with S_k = sum over the voxels entry k reads of W |F| in
                 float64, per component: what the adjointness bound between deposit and sample is stated in
rough_points(G)  the cloud the CPU and the GPU tests share: uniform, on cell faces and one ulp either side, within h / 2 of the
                 box faces (the deposit test's rough cloud without its clump), as (x, y, z) columns"""
import numpy as np

from deposit_model import REFINES, _axis32, locate

RESULT_KEYS = ("done", "served", "outside", "nonfinite")
SERVED, OUTSIDE = 0, 1
QNAN = 0x7fc00000


def sample(x, y, z, field, G, cell_size, scale=1.0):
    field = np.asarray(field, np.float32)
    M = field.shape[0]
    k = M // G
    assert k in REFINES and M == G * k and field.shape[:3] == (M, M, M) and field.ndim in (3, 4)
    N = 4 if field.ndim == 4 else 1
    F = field.reshape(M ** 3, N)
    x, y, z = (np.asarray(a, np.float32) for a in (x, y, z))
    n = len(x)
    inside = locate(x, y, z, G, cell_size) >= 0
    ax = [_axis32(s[inside], G, cell_size, k) for s in (-y, x, -z)]
    m = int(inside.sum())
    sums, S = np.zeros((m, N), np.float64), np.zeros((m, N), np.float64)           # the chains start at +0
    with np.errstate(invalid="ignore", over="ignore"):
        for d3 in (0, 1):
            for d1 in (0, 1):
                for d2 in (0, 1):
                    W1, W2, W3 = ax[0][1 + d1], ax[1][1 + d2], ax[2][1 + d3]
                    ok = (W1 != 0) & (W2 != 0) & (W3 != 0)                         # a weight of exactly 0: not read, no term
                    idx = ((ax[2][0] + d3) * M + (ax[0][0] + d1)) * M + (ax[1][0] + d2)
                    assert (idx[ok] < M ** 3).all() and (ax[0][0][ok] + d1 < M).all() and (ax[1][0][ok] + d2 < M).all()
                    W = (W1 * W2) * W3
                    v = F[np.where(ok, idx, 0)]
                    term = W[:, None] * v                                          # fp32, one rounding
                    assert W.dtype == term.dtype == np.float32
                    sums[ok] = sums[ok] + term[ok].astype(np.float64)
                    S[ok] = S[ok] + W[ok, None].astype(np.float64) * np.abs(v[ok].astype(np.float64))
        value = sums.astype(np.float32)
        words = np.float32(scale) * value
    assert words.dtype == np.float32
    out = np.full((n, N), QNAN, np.uint32).view(np.float32)
    out[inside] = words
    outcomes = np.where(inside, SERVED, OUTSIDE).astype(np.int32)
    Sfull = np.zeros((n, N), np.float64)
    Sfull[inside] = S
    res = {"done": n, "served": m, "outside": n - m, "nonfinite": int((~np.isfinite(words)).any(1).sum())}
    if N == 1:
        out, Sfull = out[:, 0], Sfull[:, 0]
    return out, outcomes, res, Sfull


def rough_points(G, cell_size=5.0, seed=3, n=(3200, 300, 300)):
    """float32 [sum(n), 3] inside the box, in (x, y, z)"""
    rng = np.random.default_rng(seed)
    cs = cell_size
    lo, hi = -(G // 2) * cs, (G - G // 2) * cs
    q = [rng.uniform(lo + 0.001, hi - 0.001, (n[0], 3))]
    face = rng.uniform(lo + 0.7, hi - 0.7, (n[1], 3)).astype(np.float32)
    planes = np.float32(cs) * rng.integers(-(G // 2) + 1, G - G // 2, n[1]).astype(np.float32)
    side = np.arange(n[1]) % 3
    planes = np.where(side == 1, np.nextafter(planes, np.float32(np.inf)), np.where(side == 2, np.nextafter(planes, np.float32(-np.inf)), planes))
    face[np.arange(n[1]), rng.integers(0, 3, n[1])] = planes
    q.append(face)
    rim = rng.uniform(lo + 0.001, hi - 0.001, (n[2], 3))
    d = rng.uniform(0.001, 0.6, n[2])
    rim[np.arange(n[2]), rng.integers(0, 3, n[2])] = np.where(np.arange(n[2]) % 2 == 0, lo + d, hi - d)
    q.append(rim)
    q = np.concatenate(q).astype(np.float32)
    return np.ascontiguousarray(np.stack([q[:, 1], -q[:, 0], -q[:, 2]], 1))


def adjoint_sides(F, sums, m, smp, S):
    """(|sum_v F_v sums_v - sum_b m_b sample_b|, sum_b m_b S_b) in float64: the two sides of the adjointness bound"""
    import math
    lhs = math.fsum((np.asarray(F, np.float64).ravel() * np.asarray(sums, np.float64).ravel()).tolist())
    rhs = math.fsum((np.asarray(m, np.float64) * np.asarray(smp, np.float64)).tolist())
    return abs(lhs - rhs), math.fsum((np.asarray(m, np.float64) * np.asarray(S, np.float64)).tolist())
