"""psamd_deposit and psamd_sample off the 5-unit 8^3 / 9^3 box (deposit.hip, sample.hip, lattice.hpp; deposit_lattice in
services.hip): other cell sizes, the smallest and the largest grids, a points launch past its block cap, frames without mass.

The comparison rules are test_gpu_deposit.py's and test_gpu_sample.py's, unchanged.  Deposit: every voxel within 1 ulp of
the fp32 model of tests/deposit_model.py fed with the frame the device built, a voxel the model has at 0 exactly +0, voxels /
bodies / skipped exact, the mass within 2^-40, vmax the largest float stored; the fp32 model within 1.75 * 4 M 2^-24 * (mass in
reach) of the plain fp64 form.  Sample: every word the model's of tests/sample_model.py bit for bit (a NaN matching a NaN), an
outside entry the quiet NaN 0x7fc00000, the outcomes and the record exact, entries at or past n untouched.

1. Cell sizes 4.0 (inv_h exact), 3.3 and 0.7 (neither they nor inv_h a float) on 8^3 cells.  The configuration keeps
   cell_size as a double and the models are given that double, float(g.cfg.cell_size), as deposit_lattice is.
2. Grids: 3^3 cells (chunk_factor 1, chunk_dim 3) -- the smallest psamd_create accepts: chunk_dim 2 is refused -- which is
   also the odd, uncentred one: every voxel is a box-edge voxel, k_deposit launches 7 workgroups at refine 1 and 2; 24^3 cells
   (884 736 voxels and 110 592 tasks at refine 4), alone and as two slabs whose cut lends a layer; 40^3 cells of 2.5
   (160^3 voxels at refine 4) with the far corner voxel sampled.
3. The points form past k_sample's cap of 2048 * 256 lanes: 524 497 entries, a second trip of three full waves and one of 17.
4. A frame without a particle (never filled; emptied by psamd_remove), and one particle alone in a corner cell.

The clouds and points are rough_cloud of test_gpu_deposit.py and rough_points of sample_model.py with every length stated in
cells (their 0.001, 0.6, 0.7 of a 5-unit cell become cell_size / 5 times that), so that the bodies on cell faces and one ulp
beside them, those within h / 2 of the box faces, the clump and the voxel centres keep their places in a box of any size."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import deposit_model as D
import particlesystem_amd as ps
import sample_model as S
from particlesystem_amd import slab
from service_harness import DEV, ERR_INVALID_ARG, bits, captured, dev, dev_read, open_frame

pytestmark = pytest.mark.gpu

GRIDS = {3: dict(max_particles_num=2048, chunk_factor=1, chunk_dim=3),                      # lists of 152
         8: dict(max_particles_num=16384, chunk_factor=2, chunk_dim=4),                      # lists of 66
         24: dict(max_particles_num=16384, chunk_factor=6, chunk_dim=4, x_factor=8),         # lists of 16 (far_harness.GRID)
         40: dict(max_particles_num=16384, chunk_factor=10, chunk_dim=4, x_factor=8)}        # lists of 8
UNIFORM = {3: (600, 100, 100), 8: (3200, 300, 300), 24: (3200, 300, 300), 40: (3200, 300, 300)}      # rough_xyz's n: 3^3 holds less
QUIET = dict(collision_radius=1e-6, drag=0.0)          # nothing collides
NAN_FILL = 0x7fc0dead                                # what neither service writes
SAMPLE_CAP = 2048 * 256                              # SAMPLE_MAX_BLOCKS * SAMPLE_THREADS (sample.hip): the points launch's lanes
PAST = 137                                           # entries of points() that a device count leaves out
# (cells, cell size) of every context with a rough cloud
SIZES = [(8, 4.0), (8, 3.3), (8, 0.7)]
EXTREMES = [(3, 5.0, 1), (3, 5.0, 2), (3, 5.0, 4), (24, 5.0, 1), (24, 5.0, 2), (24, 5.0, 4), (40, 2.5, 1), (40, 2.5, 4)]


# ---- clouds, points, lattices ---------------------------------------------------------------------------------------------------

def clump_cell(G):
    return min(2, G - 1), min(3, G - 1), min(1, G - 1)


def rough_xyz(G, cs, seed=3, n=(3200, 300, 300), clump=0):
    """float32 [sum(n) + clump, 3] in (x, y, z), drawn in cell-axis coordinates q = (-y, x, -z): a uniform cloud; bodies on the
    float nearest a cell face and one ulp either side of it; bodies within 0.12 cells of a box face (past the outermost voxel
    centres of every refine: h / 2 is an eighth of a cell at refine 4); a clump of `clump` bodies in one cell"""
    rng = np.random.default_rng(seed)
    u = cs / 5.0
    lo, hi = -(G // 2) * cs, (G - G // 2) * cs
    q = [rng.uniform(lo + 0.001 * u, hi - 0.001 * u, (n[0], 3))]
    face = rng.uniform(lo + 0.7 * u, hi - 0.7 * u, (n[1], 3)).astype(np.float32)
    planes = (cs * rng.integers(-(G // 2) + 1, G - G // 2, n[1])).astype(np.float32)
    side = np.arange(n[1]) % 3
    planes = np.where(side == 1, np.nextafter(planes, np.float32(np.inf)), np.where(side == 2, np.nextafter(planes, np.float32(-np.inf)), planes))
    face[np.arange(n[1]), rng.integers(0, 3, n[1])] = planes
    q.append(face)
    rim = rng.uniform(lo + 0.001 * u, hi - 0.001 * u, (n[2], 3))
    d = rng.uniform(0.001 * u, 0.6 * u, n[2])
    rim[np.arange(n[2]), rng.integers(0, 3, n[2])] = np.where(np.arange(n[2]) % 2 == 0, lo + d, hi - d)
    q.append(rim)
    if clump:
        q.append(lo + cs * np.array(clump_cell(G)) + rng.uniform(0.05 * u, 4.95 * u, (clump, 3)))
    q = np.concatenate(q).astype(np.float32)
    return np.ascontiguousarray(np.stack([q[:, 1], -q[:, 0], -q[:, 2]], 1))


def rough_cloud(G, cs, cap, seed=3):
    """(xyz, age, w): rough_xyz with a clump of twelve more than a cell's list holds; every 17th a kid, every 29th massless"""
    xyz = rough_xyz(G, cs, seed, UNIFORM[G], clump=cap + 12)
    rng = np.random.default_rng(seed + 1000)
    n = len(xyz)
    age = np.full(n, 3.0, np.float32)
    age[::17] = 0.5
    w = rng.uniform(20.0, 100.0, n).astype(np.float32)
    w[::29] = 0.0
    return xyz, age, w


def q_to_xyz(q):
    q = np.asarray(q, np.float32).reshape(-1, 3)
    return np.stack([q[:, 1], -q[:, 0], -q[:, 2]], 1)


def points(G, cs, seed=3):
    """pos4 of about 3 000 points (3^3: 1 000): rough_xyz without the clump; exactly on voxel centres of every refine, the first
    and the last centre of all three axes among them (the corner voxels), and beyond those in the corners; on every box face,
    one ulp inside and one ulp beyond it; outside the box by up to 0.6 cells; NaN, +-inf, 1e30 -- shuffled, and PAST uniform
    points behind them for the entries past a device count"""
    rng = np.random.default_rng(seed + 50)
    lo, hi = np.float32(-(G // 2) * cs), np.float32((G - G // 2) * cs)
    mid = np.float32(0.5 * (float(lo) + float(hi)))
    n = UNIFORM[G]
    xyz = [rough_xyz(G, cs, seed, (n[0] * 5 // 8, n[1], n[2]))]
    for k in D.REFINES:
        c = D.centres(G, cs, k).astype(np.float32)
        at = rng.integers(0, G * k, (80, 3))
        xyz.append(q_to_xyz(c[at]))
        xyz.append(q_to_xyz([[c[-1]] * 3, [c[0]] * 3, [c[-1], c[0], c[-1]]]))
    corner = np.float32(0.03 * cs)
    xyz.append(q_to_xyz([[hi - corner] * 3, [lo + corner] * 3]))
    faces = []
    for axis in range(3):
        for v in (lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf)),
                  hi, np.nextafter(hi, np.float32(np.inf)), np.nextafter(hi, np.float32(-np.inf))):
            q = np.full(3, mid, np.float32)
            q[axis] = v
            faces.append(q)
    xyz.append(q_to_xyz(faces))
    out = rng.uniform(lo, hi, (150, 3)).astype(np.float32)
    far = rng.uniform(0.0002 * cs, 0.6 * cs, 150)
    out[np.arange(150), rng.integers(0, 3, 150)] = np.where(np.arange(150) % 2 == 0, hi + far, lo - far)
    xyz.append(q_to_xyz(out))
    odd = rng.uniform(lo, hi, (24, 3)).astype(np.float32)
    odd[np.arange(24), np.arange(24) % 3] = np.tile(np.array([np.nan, np.inf, -np.inf, 1e30], np.float32), 6)
    xyz.append(odd)
    xyz = np.concatenate(xyz).astype(np.float32)
    xyz = np.concatenate([xyz[rng.permutation(len(xyz))], rough_xyz(G, cs, seed + 1, (PAST, 0, 0))])
    return np.ascontiguousarray(np.concatenate([xyz, rng.uniform(1, 2, (len(xyz), 1)).astype(np.float32)], 1))


def lattice(G, refine, vec4, seed=7):
    """a random normal field with -0, a denormal and a few NaN / inf words planted: test_gpu_sample.py's 40 of them, 5 where the
    lattice has fewer than a thousand words (3^3 cells)"""
    M = G * refine
    rng = np.random.default_rng(seed + 10 * refine + G)
    F = rng.standard_normal((M, M, M, 4) if vec4 else (M, M, M), dtype=np.float32)
    flat = F.reshape(-1)
    a, b, c, d, e = (10, 20, 28, 34, 40) if flat.size >= 1000 else (1, 2, 3, 4, 5)
    at = rng.choice(flat.size, e, replace=False)
    flat[at[:a]] = -0.0
    flat[at[a:b]] = np.float32(1e-41)
    flat[at[b:c]] = np.nan
    flat[at[c:d]] = np.inf
    flat[at[d:e]] = -np.inf
    return F


def sentinels(m, vec4):
    return torch.from_numpy(np.full((m, 4) if vec4 else (m,), NAN_FILL, np.uint32).view(np.float32)).to(DEV)


# ---- contexts ---------------------------------------------------------------------------------------------------------------------

def context(G, cs, **over):
    g = ps.ParticleSystem(ps.default_config(cell_size=cs, **{**GRIDS[G], **QUIET, **over}))
    assert g.sizes.grid_dim == G and float(g.cfg.cell_size) == cs
    return g


def snapshot(g):
    """the frame build_grid left on one context: x, y, z, w_eff by sorted index and cell_start"""
    g.synchronize()
    v = g.device_view()
    start = dev_read(v.cell_start, g.sizes.num_cells + 1, np.int32)
    n = int(start[-1])
    if n == 0:
        return (np.zeros(0, np.float32),) * 4 + (start,)
    x, y, z, w = (dev_read(v.snap_soa + 4 * k * v.sorted_cap, n, np.float32) for k in range(4))
    return x, y, z, w, start


@pytest.fixture(scope="module")
def built():
    """per (cells, cell size) one context with the rough cloud and its frame built -- one listed body outside the clump given an
    infinite mass -- and the frame read back"""
    made = {}

    def get(G, cs):
        if (G, cs) not in made:
            g = context(G, cs)
            cap = g.sizes.max_per_cell
            xyz, age, w = rough_cloud(G, cs, cap)
            ids = g.fill_particles(xyz, age=age, w=w, fert_age=np.float32(1e6))
            assert (ids >= 0).all()
            p = g.download_particles()
            live = np.nonzero(p["cell"] >= 0)[0]
            per_cell = np.bincount(p["cell"][live], minlength=G ** 3)
            c1, c2, c3 = clump_cell(G)
            calm = np.ones(len(live), bool)
            for name in ("x", "y", "z"):
                calm &= np.abs(p[name][live]) < 0.9 * (G // 2) * cs              # (an upload checks |x| against half the box)
            ok = calm & (p["cell"][live] != (c3 * G + c1) * G + c2) & (per_cell[p["cell"][live]] <= cap) & (p["age"][live] > 1.0)
            b = int(live[np.nonzero(ok)[0][7]])
            p["w"][b] = np.inf
            g.upload_particles(p[b:b + 1], first=b)
            open_frame(g)
            made[(G, cs)] = (g, snapshot(g))
        return made[(G, cs)]
    yield get
    for g, _ in made.values():
        g.close()


@pytest.fixture(scope="module")
def pts():
    made = {}

    def get(G, cs):
        if (G, cs) not in made:
            made[(G, cs)] = points(G, cs)
        return made[(G, cs)]
    return get


# ---- the two comparisons ------------------------------------------------------------------------------------------------------------

def check_deposit(g, snap, refine, bodies_above, skipped, overflow=True):
    """test_gpu_deposit.py's test_device_against_the_model on this context's frame; returns (the model's bits, the record)"""
    G, cs, cap = g.sizes.grid_dim, float(g.cfg.cell_size), g.sizes.max_per_cell
    M = G * refine
    want = D.deposit(*snap, G, cs, cap, refine)
    assert want["skipped"] == skipped and want["bodies"] > bodies_above
    counts = np.diff(snap[4])
    if overflow:
        assert counts.max() > cap or g.counters["cell_overflow_kills"] >= 12, "no list was cut at max_per_cell"
    out = torch.from_numpy(np.full((M, M, M), NAN_FILL, np.uint32).view(np.float32)).to(DEV)
    got, res = g.deposit(refine, out=out, result=True)
    assert tuple(got.shape) == (M, M, M)
    gb, wb = bits(got).astype(np.int64), bits(want["rho"]).astype(np.int64)
    ulp = np.abs(gb - wb)
    rel = abs(res["mass"] - want["mass"]) / want["mass"]
    print("%d^3 cells of %r, refine %d: %d voxels with mass of %d, %d differ by 1 ulp, none by more: %s; mass %.9g, relative error %.3g"
          % (G, cs, refine, (wb != 0).sum(), M ** 3, (ulp == 1).sum(), ulp.max() <= 1, res["mass"], rel))
    assert ulp.max() <= 1
    assert (gb[wb == 0] == 0).all(), "a voxel the model has at 0 is not +0"
    assert (res["voxels"], res["bodies"], res["skipped"]) == (M ** 3, want["bodies"], want["skipped"])
    assert rel <= 2.0 ** -40
    assert res["vmax"] == float(got.max().item()) and res == g.deposit_result()
    host, hres = g.download_deposit(refine)                       # the host form is the same pass
    assert np.array_equal(bits(host), bits(got)) and hres == res
    # accuracy: the plain fp64 form, within the bound of u's rounding
    exact = D.deposit(*snap, G, cs, cap, refine, exact=True)
    err, bound = np.abs(want["sums"] - exact["sums"]), 4.0 * M * 2.0 ** -24 * exact["support"]
    print("   fp32 model against the fp64 form: largest error / (4 M 2^-24 mass in reach) %.3g" % (err[bound > 0] / bound[bound > 0]).max())
    assert (err <= 1.75 * bound).all()
    return wb, res


def same_words(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaNs differ at", np.nonzero(gn != wn)[0][:8])
    bad = (bits(got) != bits(want)) & ~wn
    assert not bad.any(), (what, "words differ at", np.argwhere(bad)[:8], got[bad][:4], want[bad][:4])


def check_sample(g, pos4, F, n, what, scale=1.75):
    """test_gpu_sample.py's test_device_against_the_model: the first n of pos4's entries through a device count, the rest of
    out holding what it held; returns the model's (words, outcomes, record)"""
    G, cs = g.sizes.grid_dim, float(g.cfg.cell_size)
    m, vec4 = len(pos4), F.ndim == 4
    want, w_oc, w_res, _ = S.sample(pos4[:n, 0], pos4[:n, 1], pos4[:n, 2], F, G, cs, scale=scale)
    out = sentinels(m, vec4)
    count = torch.full((1,), n, dtype=torch.int64, device=DEV)
    got, oc, res = g.sample(dev(F), pos4=dev(pos4), count=count, scale=scale, out=out, outcome=True, result=True)
    got, oc = got.cpu().numpy(), oc.cpu().numpy()
    same_words(got[:n], want, what)
    assert (bits(got[:n][w_oc == 1]) == S.QNAN).all(), "an outside entry's words are not the quiet NaN 0x7fc00000"
    assert (bits(got[n:]) == NAN_FILL).all(), "entries at or past n were touched"
    assert np.array_equal(oc[:n], w_oc) and (oc[n:] == -1).all()
    assert res == w_res and g.sample_result() == res
    assert res["served"] + res["outside"] == res["done"] == n
    return want, w_oc, w_res


# ---- 1. cell sizes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("refine", D.REFINES)
@pytest.mark.parametrize("G,cs", SIZES)
def test_deposit_at_other_cell_sizes(built, G, cs, refine):
    g, snap = built(G, cs)
    assert float(g.cfg.cell_size) != 5.0
    inv_h = refine / float(g.cfg.cell_size)
    assert (float(np.float32(inv_h)) == inv_h) == (cs == 4.0)          # 4.0: inv_h is exact; 3.3 and 0.7: it is rounded
    check_deposit(g, snap, refine, 3700, 1)


@pytest.mark.parametrize("vec4", [False, True])
@pytest.mark.parametrize("refine", D.REFINES)
@pytest.mark.parametrize("G,cs", SIZES)
def test_sample_at_other_cell_sizes(built, pts, G, cs, refine, vec4):
    g, pos4 = built(G, cs)[0], pts(G, cs)
    assert float(g.cfg.cell_size) != 5.0
    _, _, res = check_sample(g, pos4, lattice(G, refine, vec4), len(pos4) - PAST, "%d^3 of %r refine %d vec4 %s" % (G, cs, refine, vec4))
    assert res["outside"] > 150 and res["nonfinite"] > 0 and res["served"] > 2500


# ---- 2. the grid's extremes -----------------------------------------------------------------------------------------------------------

def reached(g, refine):
    """what the shape is there for"""
    G, cells = g.sizes.grid_dim, g.sizes.num_cells
    tasks = cells * (8 if refine == 4 else 1)
    if G <= 3:
        assert (tasks + 3) // 4 < 8 or refine == 4          # fewer workgroups than XCDs at refine 1 and 2
    else:
        assert cells > 8192
    return tasks


@pytest.mark.parametrize("G,cs,refine", EXTREMES)
def test_deposit_at_the_grids_extremes(built, G, cs, refine):
    """3^3 cells (chunk_factor 1, chunk_dim 3) is the smallest grid: psamd_create refuses chunk_dim 2"""
    if G == 3:
        with pytest.raises(ps.PsamdError) as e:
            ps.ParticleSystem(ps.default_config(chunk_factor=1, chunk_dim=2, max_particles_num=2048))
        assert e.value.status == ERR_INVALID_ARG
    g, snap = built(G, cs)
    tasks = reached(g, refine)
    assert g.sizes.grid_dim <= 3 or g.sizes.num_cells > 8192
    counts = np.diff(snap[4])
    assert counts.max() > g.sizes.max_per_cell or g.counters["cell_overflow_kills"] >= 12      # a list was cut at max_per_cell
    wb, res = check_deposit(g, snap, refine, 800 if G == 3 else 3700, 1)
    M = G * refine
    if refine == 4:
        assert (tasks, res["voxels"]) == (G ** 3 * 8, M ** 3)
    if G > 3 and refine == 4:
        assert (wb == 0).sum() > M ** 3 * 9 // 10, "most cells are empty: most voxels are +0"
    if G == 24 and refine == 4:
        assert (M ** 3, tasks) == (884736, 110592)
    if G == 40 and refine == 4:
        assert M ** 3 * 4 == 16384000                              # a 16 MB lattice


@pytest.mark.parametrize("vec4", [False, True])
@pytest.mark.parametrize("G,cs,refine", EXTREMES)
def test_sample_at_the_grids_extremes(built, pts, G, cs, refine, vec4):
    g, pos4 = built(G, cs)[0], pts(G, cs)
    reached(g, refine)
    M = G * refine
    n = len(pos4) - PAST
    F = lattice(G, refine, vec4)
    _, w_oc, res = check_sample(g, pos4, F, n, "%d^3 of %r refine %d vec4 %s" % (G, cs, refine, vec4))
    assert res["outside"] > 150 and res["served"] > (700 if G == 3 else 2500)
    # the corner voxels are read: served entries with n0 == M - 1 on all three axes (the far corner: the last word of the
    # lattice), and with n0 == 0 on all three
    x, y, z = pos4[:n, 0], pos4[:n, 1], pos4[:n, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        n0 = [D._axis32(s, G, cs, refine)[0] for s in (-y, x, -z)]
    served = w_oc == 0
    assert (served & (n0[0] == M - 1) & (n0[1] == M - 1) & (n0[2] == M - 1)).sum() >= 2
    assert (served & (n0[0] == 0) & (n0[1] == 0) & (n0[2] == 0)).sum() >= 2
    # points on and beyond every box face (points(): the faces themselves, one ulp inside, one ulp beyond)
    lo, hi = np.float32(-(G // 2) * cs), np.float32((G - G // 2) * cs)
    for s in (-y, x, -z):
        assert (served & (s == lo)).any() and (~served & (s == hi)).any() and (~served & (s == np.nextafter(lo, np.float32(-np.inf)))).any()
        assert (served & (s == np.nextafter(hi, np.float32(-np.inf)))).any()


def slab_cloud(G, n, seed=61):
    rng = np.random.default_rng(seed)
    half = G * 2.5 * 0.9995
    return dict(xyz=rng.uniform(-half, half, (n, 3)).astype(np.float32), age=rng.uniform(0.2, 9.0, n).astype(np.float32),
                w=rng.uniform(20.0, 100.0, n).astype(np.float32), fert_age=np.float32(1e6), vxyz=rng.uniform(-8, 8, (n, 3)).astype(np.float32))


def test_two_slabs_that_lend_a_layer_give_the_single_context_bytes_on_24_cubed_cells(pts):
    """refine 4: every rank's voxels into an array of its own, prefilled -- no voxel written twice, every voxel once, the
    single context's bytes, the records merged (test_gpu_deposit.py's union_of); every rank samples the single context's words"""
    G, refine, cuts = 24, 4, [0, 10, 24]                           # rank 1 computes layer 10 of rank 0's state
    M = G * refine
    inputs = slab_cloud(G, 4000)
    one = ps.ParticleSystem(ps.default_config(**GRIDS[G]))
    one.fill_particles(**inputs)
    ranks = [ps.ParticleSystem(ps.default_config(rank=r, world=2, cuts=cuts, **GRIDS[G])) for r in range(2)]
    plans = [s.slab_plan() for s in ranks]
    assert one.sizes.num_cells > 8192 and any(p.lentin_hi > p.lentin_lo for p in plans), "no rank was lent a layer"
    for s in ranks:
        s.fill_particles(**inputs)
    open_frame(one)
    slab.to_pairs(ranks)
    want, res = one.deposit(refine, result=True)
    assert res["voxels"] == M ** 3 == 884736 and res["bodies"] > 3000 and res["mass"] > 0
    union = np.full(M ** 3, NAN_FILL, np.uint32)
    recs, hosts = [], []
    for s in ranks:
        out = torch.from_numpy(np.full((M, M, M), NAN_FILL, np.uint32).view(np.float32)).to(DEV)
        got, r = s.deposit(refine, out=out, result=True)
        b = bits(got).ravel()
        wrote = b != NAN_FILL
        assert wrote.sum() == r["voxels"] and (union[wrote] == NAN_FILL).all(), "a voxel was written by two ranks"
        union[wrote] = b[wrote]
        recs.append(r)
        host, hr = s.download_deposit(refine)
        assert hr == r and np.array_equal(bits(host).ravel()[wrote], b[wrote]) and (bits(host).ravel()[~wrote] == 0).all()
        hosts.append(host)
    assert (union != NAN_FILL).all(), "a voxel was written by no rank"
    assert np.array_equal(union, bits(want).ravel()), "the ranks' voxels differ from the single context's"
    merged = ps.merge_deposit(recs)
    assert {k: merged[k] for k in ("voxels", "bodies", "skipped", "vmax")} == {k: res[k] for k in ("voxels", "bodies", "skipped", "vmax")}
    assert abs(merged["mass"] - res["mass"]) <= 2.0 ** -40 * res["mass"], (merged, res)
    assert np.array_equal(bits(hosts[0] + hosts[1]), bits(want))
    # the deposit itself as the field: every rank, given all points, returns the single context's words
    pos4 = dev(pts(G, 5.0))
    smp, oc, sres = one.sample(want, pos4=pos4, outcome=True, result=True)
    assert sres["served"] > 2500
    for s in ranks:
        got, goc, gres = s.sample(want, pos4=pos4, outcome=True, result=True)
        assert bits(got).tobytes() == bits(smp).tobytes() and torch.equal(goc, oc) and gres == sres
    one.calc_forces()
    slab.apply_stage(ranks)
    slab.finish_stage(ranks)
    assert sum(s.live_count() for s in ranks) == one.live_count() > 3000        # the step went on
    one.close()
    for s in ranks:
        s.close()


# ---- 3. past the sample launch's cap ------------------------------------------------------------------------------------------------

def spoil(F, rng, count=12):
    """`count` inner voxels (n1, n2, n3) of the lattice given a NaN or an infinity"""
    at = rng.integers(1, F.shape[0] - 1, (count, 3))
    F[at[:, 2], at[:, 0], at[:, 1]] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), count).reshape((count,) + (1,) * (F.ndim - 3))
    return at


def plant(rows, xyz, spoilt, G, cs, refine, rng):
    """among the entries `rows` (200 or more): 70 outside the box, 8 at positions that are no numbers, 40 within 0.4 h of the
    centre of a spoilt voxel"""
    lo, hi = -(G // 2) * cs, (G - G // 2) * cs
    a, b, d = rows[:70], rows[70:78], rows[78:118]
    far = rng.uniform(0.001 * cs, 2.0 * cs, 70)
    xyz[a, rng.integers(0, 3, 70)] = np.where(np.arange(70) % 2 == 0, hi + far, lo - far).astype(np.float32)      # (x, y and z range alike on an even grid)
    xyz[b, np.arange(8) % 3] = np.tile(np.array([np.nan, np.inf, -np.inf, 1e30], np.float32), 2)
    at = spoilt[np.arange(40) % len(spoilt)]
    xyz[d] = q_to_xyz(D.centres(G, cs, refine)[at] + rng.uniform(-0.4, 0.4, (40, 3)) * (cs / refine))


@pytest.mark.parametrize("vec4", [False, True])
def test_the_points_form_past_the_launch_cap(built, vec4):
    """n = 2048 * 256 + 3 * 64 + 17 entries: block 0's four waves make a second trip, three of them full and one of 17 lanes.
    (The second trip holds 209 entries, so the few hundred planted outside points are split: 70 in the second trip, 70 in
    block 0's first trip -- the same waves' counts then come from both trips -- and 300 over the rest of the first.)"""
    G, refine = 8, 2
    g = built(G, 4.0)[0]
    cs = float(g.cfg.cell_size)
    n = SAMPLE_CAP + 3 * 64 + 17
    m = n + 100
    assert n > 2048 * 256 and n - SAMPLE_CAP == 209
    rng = np.random.default_rng(77)
    half = (G // 2) * cs
    xyz = rng.uniform(-half, half, (m, 3)).astype(np.float32)
    F = lattice(G, refine, vec4)
    tail, head = np.arange(SAMPLE_CAP, n), np.arange(0, 256)
    spoilt = spoil(F, rng)
    plant(tail, xyz, spoilt, G, cs, refine, rng)
    plant(head, xyz, spoilt, G, cs, refine, rng)
    rest = rng.choice(np.arange(256, SAMPLE_CAP), 300, replace=False)
    xyz[rest, rng.integers(0, 3, 300)] = (half + rng.uniform(0.001, 3.0, 300)).astype(np.float32) * np.where(np.arange(300) % 2 == 0, 1, -1).astype(np.float32)
    pos4 = np.ascontiguousarray(np.concatenate([xyz, np.ones((m, 1), np.float32)], 1))
    want, w_oc, res = check_sample(g, pos4, F, n, "past the cap, vec4 %s" % vec4)
    assert res["served"] + res["outside"] == n and res["done"] == n
    # both trips have entries of every kind: the record's counts are sums over the trips
    nonfinite = (~np.isfinite(want.reshape(n, -1))).any(1) & (w_oc == 0)
    for rows in (tail, head):
        assert (w_oc[rows] == 1).sum() >= 78 and (w_oc[rows] == 0).sum() >= 100 and nonfinite[rows].sum() >= 30
    assert res["nonfinite"] == nonfinite.sum() and res["outside"] >= 2 * 78 + 300


# ---- 4. empty and nearly empty frames -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def empty():
    """two contexts of 8^3 cells whose frame holds no particle: one never filled, one emptied by psamd_remove"""
    never, emptied = context(8, 5.0), context(8, 5.0)
    emptied.fill_particles(rough_xyz(8, 5.0, 5, (50, 0, 0)), age=np.float32(3.0), fert_age=np.float32(1e6))
    assert emptied.live_count() == 50
    r = emptied.remove(box=((-1e30,) * 3, (1e30,) * 3))
    assert r["removed"] == 50 and emptied.live_count() == 0
    for g in (never, emptied):
        open_frame(g)
    yield {"never filled": never, "emptied": emptied}
    never.close()
    emptied.close()


@pytest.mark.parametrize("kind", ["never filled", "emptied"])
def test_deposit_on_a_frame_without_a_particle(empty, kind):
    """every voxel is written and is +0, so vmax -- the largest float written, -inf only where none is -- is +0"""
    g = empty[kind]
    snap = snapshot(g)
    assert g.live_count() == 0 and int(snap[4][-1]) == 0
    for refine in D.REFINES:
        M = 8 * refine
        out = torch.from_numpy(np.full((M, M, M), NAN_FILL, np.uint32).view(np.float32)).to(DEV)
        got, res = g.deposit(refine, out=out, result=True)
        assert (bits(got) == 0).all(), "a voxel of an empty frame is not +0"
        assert res == dict(voxels=M ** 3, bodies=0, skipped=0, mass=0.0, vmax=0.0) == g.deposit_result()
        assert math.copysign(1.0, res["mass"]) == 1.0 and math.copysign(1.0, res["vmax"]) == 1.0
        want = D.deposit(*snap, 8, 5.0, g.sizes.max_per_cell, refine)
        assert {k: want[k] for k in D.RESULT_KEYS} == res and not bits(want["rho"]).any()
        host, hres = g.download_deposit(refine)
        assert not bits(host).any() and hres == res


@pytest.mark.parametrize("kind", ["never filled", "emptied"])
def test_sample_by_export_order_without_a_live_particle(empty, kind):
    g = empty[kind]
    slots = g.owned_slots()
    assert g.live_count() == 0 and slots > 1000
    zero = dict(done=0, served=0, outside=0, nonfinite=0)
    for vec4 in (False, True):
        F = dev(lattice(8, 2, vec4))
        out = sentinels(slots, vec4)
        got, oc, res = g.sample(F, out=out, outcome=True, result=True)
        assert res == zero == g.sample_result()
        assert (bits(got) == NAN_FILL).all() and (oc == -1).all().item(), "out or the outcomes were touched"
        # captured into a caller's graph and replayed
        rec = torch.full((C.sizeof(ps.SampleResult),), 0xff, dtype=torch.uint8, device=DEV)
        spec = ps.SampleSpec(flags=int(vec4) | ps.SAMPLE_EXPORT_ORDER, refine=2, field=F.data_ptr(), capacity=16 ** 3, max_count=slots,
                             out=out.data_ptr(), scale=1.0, result_dev=rec.data_ptr())
        with captured(g) as cap:
            rc = g.lib.psamd_sample(g.h, C.byref(spec))
        assert rc == 0
        cap.launch()
        assert ps.SampleResult.from_device(rec).to_dict() == zero and (bits(out) == NAN_FILL).all()
        cap.close()


def test_one_particle_alone_in_a_corner_cell():
    G, cs = 8, 3.3
    g = context(G, cs)
    hi = (G - G // 2) * cs
    xyz = q_to_xyz([[hi - 0.3 * cs, hi - 0.45 * cs, hi - 0.2 * cs]])
    g.fill_particles(xyz, age=np.float32(3.0), w=np.float32(37.5), fert_age=np.float32(1e6))
    open_frame(g)
    snap = snapshot(g)
    counts = np.diff(snap[4])
    assert counts.sum() == 1 and counts[-1] == 1                  # the last cell: (G - 1, G - 1, G - 1)
    for refine in D.REFINES:
        wb, res = check_deposit(g, snap, refine, 0, 0, overflow=False)
        assert 1 <= (wb != 0).sum() <= 8 and res["bodies"] == 1
        assert abs(res["mass"] - 37.5) <= 2.0 ** -21 * 37.5
        for vec4 in (False, True):
            F = lattice(G, refine, vec4)
            want, w_oc, w_res, _ = S.sample(xyz[:, 0], xyz[:, 1], xyz[:, 2], F, G, cs)
            out = sentinels(g.owned_slots(), vec4)
            got, oc, sres = g.sample(dev(F), out=out, outcome=True, result=True)
            assert sres == w_res == dict(done=1, served=1, outside=0, nonfinite=w_res["nonfinite"])
            same_words(got[:1].cpu().numpy(), want, "the particle's own position")
            assert (bits(got[1:]) == NAN_FILL).all() and int(oc[0]) == 0 and (oc[1:] == -1).all().item()
    g.close()
