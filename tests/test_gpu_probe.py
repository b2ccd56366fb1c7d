"""The field at chosen points on the device (psamd_probe / psamd_probe_result_get, probe.hip).

What pins the arithmetic: a probe on an adult repeats that adult's force record bit for bit (cutoff contexts, exact
path); a probe on a kid's true position repeats that kid's phi from psamd_potential bit for bit; a slab world's merged
probes are the single context's bytes.  Everything else is held against an fp64 direct sum formed here with numpy from
the downloaded fp32 positions, ages (a kid has mass 0), masses and cell lists over the stencil that the locate rule
(Geometry::locate, the fp64 floor test) assigns to the point:
    a(x) = s * sum_j w_j (x_j - x) / (|x_j - x|^2 + eps2)^(3/2),    phi(x) = - s * sum_j w_j / sqrt(|x_j - x|^2 + eps2)
with the project's 1e-5 bound (BASELINE north star; tests/test_gpu_extras.py, tests/test_gpu_potential.py): phi relative
to |phi| (masses share a sign, nothing cancels), the acceleration relative to S = sum_j |term_j|, so that cancellation
does not make the bound vacuous.  Shapes: the 8^3 grid of tests/test_gpu_potential.py unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest
import torch

import particlesystem_amd as ps
from particlesystem_amd import slab
from service_harness import DEV, ERR_INVALID_ARG, ERR_STATE, ERR_UNSUPPORTED, bits, captured, kid_age, open_frame, slab_inputs
from util import cloud

pytestmark = pytest.mark.gpu

REL = 1e-5
SMALL = dict(chunk_factor=2, chunk_dim=4)          # an 8^3 grid of 5-unit cells: the box is [-20, 20)^3
QUIET = dict(collision_radius=0.0, drag=0.0)       # nothing collides: every adult gets a force record
QNAN = 0x7fc00000


def dev4(xyz):
    p = np.zeros((len(xyz), 4), np.float32)
    p[:, :3] = xyz
    p[:, 3] = 7.0                                   # w is ignored
    return torch.from_numpy(p).to(DEV)


def cell_points(rng, cell, n, G=8, cs=5.0):
    """n points inside cell (i1, i2, i3): i2 ~ +x, i1 ~ -y, i3 ~ -z"""
    i1, i2, i3 = cell
    u = rng.uniform(0.1, cs - 0.1, (n, 3))
    return np.stack([(i2 - G // 2) * cs + u[:, 0], -((i1 - G // 2) * cs + u[:, 1]), -((i3 - G // 2) * cs + u[:, 2])], 1).astype(np.float32)


COUNTS = (1, 7, 8, 9, 63, 64, 65)                   # the group-of-eight boundaries, the chain and slice boundary


def boundary_cloud(seed=5):
    """about 1 500 particles in 49 cells of the 8^3 grid holding 1, 7, 8, 9, 63, 64 and 65 bodies (the others none): the
    eight corners, cells on edges and faces (truncated stencils), a block inside; every 53rd particle a kid"""
    rng = np.random.default_rng(seed)
    cells = [(a, b, c) for a in (0, 7) for b in (0, 7) for c in (0, 7)]
    cells += [(i, 0, 0) for i in range(1, 7)] + [(0, i, 7) for i in range(1, 7)]
    cells += [(0, a, b) for a in (3, 4) for b in (3, 4)] + [(a, b, 7) for a in (3, 4) for b in (3, 4)]
    cells += [(a, b, c) for a in (3, 4, 5) for b in (3, 4, 5) for c in (3, 4, 5)][:21]
    assert len(cells) == 49 == len(set(cells))
    xyz = np.concatenate([cell_points(rng, c, COUNTS[(k * 3 + k // 7) % 7]) for k, c in enumerate(cells)])
    age = np.full(len(xyz), 3.0, np.float32)
    age[::53] = 0.5
    w = rng.uniform(20.0, 100.0, len(xyz)).astype(np.float32)
    return xyz, age, w


def system(xyz, age, w, **over):
    g = ps.ParticleSystem(ps.default_config(**{**SMALL, **QUIET, **over}))
    g.fill_particles(xyz, age=age, w=w, fert_age=np.float32(1e6))
    return g


def locate(xyz, G, cs):
    """Geometry::locate on float32 points: (global cell or -1)"""
    p = np.asarray(xyz, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        d1, d2, d3 = np.floor(-p[:, 1] / cs) + G // 2, np.floor(p[:, 0] / cs) + G // 2, np.floor(-p[:, 2] / cs) + G // 2
        ok = (d1 >= 0) & (d1 < G) & (d2 >= 0) & (d2 < G) & (d3 >= 0) & (d3 < G)
    cell = np.full(len(p), -1, np.int64)
    cell[ok] = ((d3[ok] * G + d1[ok]) * G + d2[ok]).astype(np.int64)
    return cell


class Ref:
    """the fp64 direct sum over a built frame (Frame.phi_of of tests/test_gpu_potential.py, restated for points)"""

    def __init__(self, g):
        p, cg = g.download_particles(), g.download_cellgrid()
        self.G, self.cs, self.eps2 = g.sizes.grid_dim, float(g.cfg.cell_size), float(g.cfg.eps2)
        self.s = -1.0 if g.cfg.force_sign < 0 else 1.0
        self.xyz = np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float64)
        self.w = np.where(p["age"].astype(np.float64) < kid_age(g.cfg), 0.0, p["w"].astype(np.float64))
        self.count, self.lists = cg[:, 0].astype(np.int64), cg[:, 1:]
        assert self.count.max() <= g.sizes.max_per_cell
        self.everybody = np.concatenate([self.lists[c, :self.count[c]] for c in np.nonzero(self.count)[0]])

    def stencil_ids(self, c):
        G = self.G
        i3, r = divmod(int(c), G * G)
        i1, i2 = divmod(r, G)
        out = [np.zeros(0, np.int64)]
        for d3 in (-1, 0, 1):
            for d1 in (-1, 0, 1):
                for d2 in (-1, 0, 1):
                    j3, j1, j2 = i3 + d3, i1 + d1, i2 + d2
                    if 0 <= j3 < G and 0 <= j1 < G and 0 <= j2 < G:
                        n = (j3 * G + j1) * G + j2
                        out.append(self.lists[n, :self.count[n]])
        return np.concatenate(out).astype(np.int64)

    def field(self, points, everybody=False):
        """(cell, acc [m, 3], S [m], phi [m]) of float32 points; rows of points outside the box are NaN"""
        cell = locate(points, self.G, self.cs)
        x = np.asarray(points, np.float32).astype(np.float64)
        acc, S, phi = np.full((len(x), 3), np.nan), np.full(len(x), np.nan), np.full(len(x), np.nan)
        cache = {}
        for k in np.nonzero(cell >= 0)[0]:
            c = int(cell[k])
            if c not in cache:
                ids = self.everybody if everybody else self.stencil_ids(c)
                cache[c] = ids[self.w[ids] != 0.0]
            ids = cache[c]
            d = self.xyz[ids] - x[k]
            e = (d * d).sum(1) + self.eps2
            t = d * (self.s * self.w[ids] / (e * np.sqrt(e)))[:, None]
            acc[k], S[k] = t.sum(0), np.linalg.norm(t, axis=1).sum()
            phi[k] = -self.s * (self.w[ids] / np.sqrt(e)).sum()
        return cell, acc, S, phi


def check_direct(ref, points, out4, what, everybody=False):
    """out4 of served points against the direct sum; exact zeros where the sum has no term; prints the largest errors"""
    cell, acc, S, phi = ref.field(points, everybody)
    got = np.asarray(out4, np.float32)
    inside = cell >= 0
    empty = inside & (S == 0.0)
    assert (bits(got[empty, :3]) == 0).all() and (got[empty, 3] == 0).all(), what + ": a point with no body in reach is not +0"
    full = inside & (S > 0.0)
    ea = np.linalg.norm(got[full, :3].astype(np.float64) - acc[full], axis=1) / S[full]
    ep = np.abs(got[full, 3].astype(np.float64) - phi[full]) / np.abs(phi[full])
    print("%s: %d points with bodies in reach, %d without; largest |a - a64| / S %.3g, largest relative error of phi %.3g"
          % (what, full.sum(), empty.sum(), ea.max() if full.any() else 0.0, ep.max() if full.any() else 0.0))
    assert full.any() and ea.max() <= REL and ep.max() <= REL, (what, ea.max(), ep.max())
    return empty.sum(), full.sum()


def raw_probe(g, pos4, max_count=None, count=None, fields=3, out4=None, outcome=None, result=None, expect=0):
    """psamd_probe as the C ABI takes it, on the context's stream behind torch's; waits"""
    spec = ps.ProbeSpec(fields=fields, max_count=len(pos4) if max_count is None else max_count)
    spec.pos4 = None if pos4 is None or len(pos4) == 0 else pos4.data_ptr()
    spec.out4 = None if out4 is None else out4.data_ptr()
    spec.count_dev = None if count is None else count.data_ptr()
    spec.outcome_dev = None if outcome is None else outcome.data_ptr()
    spec.result_dev = None if result is None else result.data_ptr()
    with g._on_stream(DEV):
        rc = g.lib.psamd_probe(g.h, C.byref(spec))
    assert rc == expect, rc
    return spec


@pytest.fixture(scope="module")
def the_cloud():
    return boundary_cloud()


# ---- 1, 2: parity with the force pass and with the potential ---------------------------------------------------------------

@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("graphs", [False, True])
def test_a_probe_on_a_particle_repeats_its_force_record_and_its_potential(the_cloud, sign, graphs):
    xyz, age, w = the_cloud
    g = system(xyz, age, w, force_sign=sign)
    g.set_graphs(graphs)
    open_frame(g)
    ref = Ref(g)
    assert sorted(set(ref.count.tolist())) == [0] + list(COUNTS) and len(xyz) > 1400
    ex = g.export_live(ps.EXPORT_POS | ps.EXPORT_VEL | ps.EXPORT_ID)
    pos4 = ex["pos4"].contiguous()
    n = len(pos4)
    res = g.probe(pos4, outcome=True)
    assert (res["done"], res["served"], res["outside"], res["foreign"], res["nonfinite"]) == (n, n, 0, 0, 0)
    assert not res["outcome"].any().item()
    got = res["out4"].cpu().numpy()
    if graphs:
        # the probe itself captured on a second call (no scratch grows), replayed: the same bytes
        out2 = torch.zeros((n, 4), dtype=torch.float32, device=DEV)
        spec = ps.ProbeSpec(fields=3, max_count=n, pos4=pos4.data_ptr(), out4=out2.data_ptr())
        with captured(g) as cap:
            rc = g.lib.psamd_probe(g.h, C.byref(spec))
        assert rc == 0
        cap.launch()
        assert np.array_equal(bits(out2), bits(got))
        cap.close()
    # the potential on the same frame
    pot = g.potential(phi=True)
    phi = pot["phi"].cpu().numpy()
    assert len(phi) == n
    g.calc_forces_pairs()
    fx = g.export_live(ps.EXPORT_ACC | ps.EXPORT_VEL | ps.EXPORT_ID)
    assert np.array_equal(fx["id"].cpu().numpy(), ex["id"].cpu().numpy())
    adult = fx["vel4"].cpu().numpy()[:, 3] >= np.float32(kid_age(g.cfg))
    assert 20 < (~adult).sum() < 40
    force = fx["acc4"].cpu().numpy()[:, :3]
    assert np.abs(force[adult]).max() > 0
    wrong = np.nonzero((bits(got[:, :3]) != bits(force)).any(1) & adult)[0]
    assert len(wrong) == 0, "%d of %d adults: the probe differs from the force record, first entry %d: %r against %r" % (
        len(wrong), adult.sum(), wrong[0], got[wrong[0], :3], force[wrong[0]])
    # a kid: psamd_potential's phi bit for bit
    assert np.array_equal(bits(got[~adult, 3]), bits(phi[~adult]))
    # an adult: the fp64 direct sum that includes the own term
    cell, acc, S, phi64 = ref.field(pos4.cpu().numpy()[:, :3])
    err = np.abs(got[adult, 3].astype(np.float64) - phi64[adult]) / np.abs(phi64[adult])
    own = -sign * ex["pos4"].cpu().numpy()[adult, 3].astype(np.float64) / np.sqrt(ref.eps2)
    off = np.abs(got[adult, 3].astype(np.float64) - (phi[adult].astype(np.float64) + own)) / np.abs(phi64[adult])
    print("force_sign %+g graphs %s: %d adults equal their force records; phi of adults: largest relative error %.3g, "
          "against psamd_potential's phi plus the own term %.3g" % (sign, graphs, adult.sum(), err.max(), off.max()))
    assert err.max() <= REL and off.max() <= REL
    g.calc_forces_apply()
    g.synchronize()
    g.close()


# ---- 3: points that are no particles -----------------------------------------------------------------------------------------

def lattice_points():
    t = (np.arange(9) * 5.0 - 20.0).astype(np.float32)          # the cell faces; +20 is outside, and so is y or z = -20
    X, Y, Z = np.meshgrid(t, t, t, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1)
    near = []
    for face in (-5.0, 0.0, 5.0, 15.0):                          # one ulp either side of a face, on each axis
        for side in (-np.inf, np.inf):
            v = np.nextafter(np.float32(face), np.float32(side))
            near += [(v, 1.25, -1.25), (1.25, v, -1.25), (1.25, -1.25, v), (v, v, v)]
    return np.concatenate([pts, np.array(near, np.float32)]).astype(np.float32)


def test_lattice_nodes_on_faces_and_in_empty_cells(the_cloud):
    xyz, age, w = the_cloud
    g = system(xyz, age, w)
    open_frame(g)
    pts = lattice_points()
    res = g.probe(dev4(pts), outcome=True)
    cell = locate(pts, 8, 5.0)
    assert np.array_equal(res["outcome"].cpu().numpy(), np.where(cell >= 0, 0, 1))
    assert res["served"] == (cell >= 0).sum() and res["outside"] == (cell < 0).sum() == 9 ** 3 - 8 ** 3
    out = res["out4"].cpu().numpy()
    assert (bits(out[cell < 0]) == QNAN).all()
    empty, full = check_direct(Ref(g), pts, out, "lattice")
    assert empty > 20 and full > 200
    g.close()


# ---- 4: outcomes and counts ----------------------------------------------------------------------------------------------

def test_outcomes_counts_and_untouched_entries(the_cloud):
    xyz, age, w = the_cloud
    g = system(xyz, age, w)
    open_frame(g)
    rng = np.random.default_rng(41)
    L = np.float32(20.0)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    special = np.array([(25, 0, 0), (0, -30, 0), (0, 0, 1e30), (nan, 1, 1), (1, nan, 1), (1, 1, nan), (inf, 1, 1), (1, -inf, 1), (1, 1, inf),
                        (L, 1, 1), (-L, 1, 1), (1, L, 1), (1, -L, 1), (1, 1, L), (1, 1, -L), (-L, L, L), (L, -L, -L)], np.float32)
    pts = np.concatenate([special, rng.uniform(-20, 20, (83, 3)).astype(np.float32)])
    cell = locate(pts, 8, 5.0)
    assert cell[10] >= 0 and cell[11] >= 0 and cell[13] >= 0 and cell[15] >= 0 and (cell[[9, 12, 14, 16]] < 0).all() and (cell[:9] < 0).all()
    m = len(pts)
    pos4 = dev4(pts)
    full = g.probe(pos4, outcome=True)
    full4 = full["out4"].cpu().numpy()
    for cnt in (None, 0, -3, 1, 40, m, m + 1000):
        n = m if cnt is None else min(max(cnt, 0), m)
        out4 = torch.full((m, 4), -77.0, dtype=torch.float32, device=DEV)
        outcome = torch.full((m,), -9, dtype=torch.int32, device=DEV)
        rec = torch.zeros(C.sizeof(ps.ProbeResult), dtype=torch.uint8, device=DEV)
        count = None if cnt is None else torch.tensor([cnt], dtype=torch.int64, device=DEV)
        raw_probe(g, pos4, count=count, out4=out4, outcome=outcome, result=rec)
        got, oc = out4.cpu().numpy(), outcome.cpu().numpy()
        assert (got[n:] == -77.0).all() and (oc[n:] == -9).all(), "entries at or past n were touched (count %r)" % cnt
        assert np.array_equal(oc[:n], np.where(cell[:n] >= 0, 0, 1))
        assert np.array_equal(bits(got[:n]), bits(full4[:n]))
        assert (bits(got[:n][cell[:n] < 0]) == QNAN).all()
        served = got[:n][cell[:n] >= 0]
        want = {"done": n, "served": int((cell[:n] >= 0).sum()), "outside": int((cell[:n] < 0).sum()), "foreign": 0,
                "nonfinite": int((~np.isfinite(served)).any(1).sum())}
        assert ps.ProbeResult.from_device(rec).to_dict() == want == g.probe_result(), (cnt, want)
    # max_count 0: a zero record, nothing else
    rec = torch.full((C.sizeof(ps.ProbeResult),), 255, dtype=torch.uint8, device=DEV)
    raw_probe(g, None, max_count=0, result=rec)
    assert ps.ProbeResult.from_device(rec).to_dict() == g.probe_result() == dict.fromkeys(("done", "served", "outside", "foreign", "nonfinite"), 0)
    # acc alone, phi alone: the components that were not asked for are 0.0f
    both = full4[cell >= 0]
    only_a, only_p = g.probe(pos4, phi=False)["out4"].cpu().numpy()[cell >= 0], g.probe(pos4, acc=False)["out4"].cpu().numpy()[cell >= 0]
    assert np.array_equal(bits(only_a[:, :3]), bits(both[:, :3])) and (bits(only_a[:, 3]) == 0).all()
    assert np.array_equal(bits(only_p[:, 3]), bits(both[:, 3])) and (bits(only_p[:, :3]) == 0).all()
    # all probes in one cell (a wave's worth, one less, one more, a single one), and 64 probes in 64 cells
    ref = Ref(g)
    busy = (4, 4, 4)
    for k in (1, 63, 64, 65):
        p = cell_points(rng, busy, k)
        r = g.probe(dev4(p))
        assert r["served"] == k == r["done"]
        check_direct(ref, p, r["out4"].cpu().numpy(), "%d probes in one cell" % k)
    p = np.concatenate([cell_points(rng, (a, b, c), 1) for a in range(2, 6) for b in range(2, 6) for c in range(2, 6)])
    r = g.probe(dev4(p))
    assert r["served"] == 64 and len(set(locate(p, 8, 5.0).tolist())) == 64
    check_direct(ref, p, r["out4"].cpu().numpy(), "64 probes in 64 cells")
    g.close()


# ---- 5: independence -------------------------------------------------------------------------------------------------------

def test_a_probe_depends_on_its_position_and_the_frame_alone(the_cloud):
    xyz, age, w = the_cloud
    g = system(xyz, age, w)
    open_frame(g)
    rng = np.random.default_rng(51)
    pts = np.concatenate([xyz[::3], rng.uniform(-20, 20, (300, 3)).astype(np.float32)])
    a = g.probe(dev4(pts))["out4"].cpu().numpy()
    b = g.probe(dev4(pts))["out4"].cpu().numpy()
    assert np.array_equal(bits(a), bits(b)), "twice in a row"
    perm = rng.permutation(len(pts) + 5000)
    padded = np.concatenate([pts, rng.uniform(-25, 25, (5000, 3)).astype(np.float32)])[perm]
    c = g.probe(dev4(padded))["out4"].cpu().numpy()
    back = np.empty_like(c)
    back[perm] = c
    assert np.array_equal(bits(back[:len(pts)]), bits(a)), "shuffled and padded with others"
    big = torch.zeros((20000, 4), dtype=torch.float32, device=DEV)
    big[:len(pts)] = dev4(pts)
    out = torch.zeros((20000, 4), dtype=torch.float32, device=DEV)
    raw_probe(g, big, count=torch.tensor([len(pts)], dtype=torch.int64, device=DEV), out4=out)
    assert np.array_equal(bits(out[:len(pts)]), bits(a)), "a larger max_count"
    g.calc_forces_pairs()
    d = g.probe(dev4(pts))["out4"].cpu().numpy()
    assert np.array_equal(bits(d), bits(a)), "after the pair stage"
    g.calc_forces_apply()
    g.synchronize()
    g.close()


# ---- 6: fast math ------------------------------------------------------------------------------------------------------------

def test_fast_math_stays_within_the_bound_of_the_exact_probe(the_cloud):
    xyz, age, w = the_cloud
    out = []
    for flags in (0, ps.FLAG_FAST_MATH):
        g = system(xyz, age, w, flags=flags)
        open_frame(g)
        pos4 = g.export_live(ps.EXPORT_POS)["pos4"].contiguous()
        r = g.probe(pos4)
        assert r["served"] == len(xyz) and r["nonfinite"] == 0
        again = g.probe(pos4)
        assert np.array_equal(bits(r["out4"]), bits(again["out4"]))
        out.append(r["out4"].cpu().numpy().astype(np.float64))
        g.close()
    b, a = out
    rel = np.linalg.norm(a[:, :3] - b[:, :3], axis=1) / np.maximum(np.linalg.norm(b[:, :3], axis=1), 1e-30)
    relp = np.abs(a[:, 3] - b[:, 3]) / np.abs(b[:, 3])
    print("fast math against the exact probe: largest relative deviation of |a| %.3g, of phi %.3g" % (rel.max(), relp.max()))
    assert rel.max() < REL and relp.max() < REL


# ---- 7: all-pairs -----------------------------------------------------------------------------------------------------------

def test_all_pairs_inside_a_block_of_cells_is_the_cutoff_result():
    rng = np.random.default_rng(71)
    xyz = rng.uniform((0.1, -9.9, -9.9), (9.9, -0.1, -0.1), (1200, 3)).astype(np.float32)      # a 2x2x2 block of cells
    pts = np.concatenate([xyz[::4], rng.uniform((0, -10, -10), (10, 0, 0), (200, 3)).astype(np.float32)])
    got = []
    for flags in (0, ps.FLAG_ALL_PAIRS):
        g = system(xyz, np.float32(3.0), np.float32(60.0), flags=flags)
        open_frame(g)
        assert (Ref(g).count > 0).sum() == 8
        r = g.probe(dev4(pts))
        assert r["served"] == len(pts)
        got.append(r["out4"].cpu().numpy())
        g.close()
    assert np.array_equal(bits(got[0]), bits(got[1]))


def test_all_pairs_spread_cloud_against_the_fp64_direct_sum():
    n = 4096
    rng = np.random.default_rng(72)
    age = np.full(n, 3.0, np.float32)
    age[::31] = 0.5
    g = system(cloud(n, 73, 20.0), age, rng.uniform(20.0, 100.0, n).astype(np.float32), flags=ps.FLAG_ALL_PAIRS)
    open_frame(g)
    t = (np.arange(8) * 5.0 - 17.5).astype(np.float32)           # 512 lattice probes, the cells' centres
    X, Y, Z = np.meshgrid(t, t, t, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1)
    r = g.probe(dev4(pts))
    assert r["served"] == 512 and r["nonfinite"] == 0
    check_direct(Ref(g), pts, r["out4"].cpu().numpy(), "all-pairs, 4096 bodies, 512 probes", everybody=True)
    g.close()


# ---- 8: slabs ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cuts", [[0, 7, 16], [0, 8, 16], [0, 3, 7, 11, 16]])
def test_slabs_merge_to_the_single_context_bytes(cuts):
    n = 20000
    xyz, age, v = slab_inputs(n, 81)
    rng = np.random.default_rng(83)
    pts = np.concatenate([xyz[::10], rng.uniform(-42, 42, (1500, 3)).astype(np.float32)])
    pos4 = dev4(pts)
    inside = locate(pts, 16, 5.0) >= 0
    one = ps.ParticleSystem(ps.default_config(**QUIET))
    one.fill_particles(xyz, age=age, fert_age=np.float32(1e6), vxyz=v)
    world = len(cuts) - 1
    ranks = [ps.ParticleSystem(ps.default_config(rank=r, world=world, cuts=cuts, **QUIET)) for r in range(world)]
    if cuts == [0, 8, 16]:
        plans = [s.slab_plan() for s in ranks]
        assert plans[0].lentout_lo < plans[0].lentout_hi and plans[1].lentin_lo < plans[1].lentin_hi      # the plan the potential refuses
    for s in ranks:
        s.fill_particles(xyz, age=age, fert_age=np.float32(1e6), vxyz=v)
    for step in range(2):
        if step:
            one.step(1)
            slab.step_local(ranks)
        open_frame(one)
        want = one.probe(pos4, outcome=True)
        assert want["served"] == inside.sum() and want["foreign"] == 0
        slab.to_pairs(ranks)
        parts = [s.probe(pos4, outcome=True) for s in ranks]
        codes = np.stack([p["outcome"].cpu().numpy() for p in parts])
        assert ((codes == 0).sum(0) == inside).all(), "an in-box probe is served by exactly one rank, the others by none"
        assert ((codes == 1).all(0) == ~inside).all()
        merged = ps.merge_probe(parts)
        assert np.array_equal(bits(merged["out4"]), bits(want["out4"])), "step %d: the ranks' probes differ from the single context's" % step
        assert merged["served"] == want["served"] == sum(p["served"] for p in parts) and merged["nonfinite"] == want["nonfinite"]
        assert merged["outside"] == want["outside"] and merged["foreign"] == 0
        one.calc_forces()
        slab.apply_stage(ranks)
        slab.finish_stage(ranks)
    one.close()
    for s in ranks:
        s.close()


def test_all_pairs_slabs_are_refused_and_the_step_goes_on():
    n = 8000
    xyz, age, v = slab_inputs(n, 81)
    over = dict(flags=ps.FLAG_ALL_PAIRS, max_particles_num=1 << 18, **QUIET)
    one = ps.ParticleSystem(ps.default_config(**over))
    ranks = [ps.ParticleSystem(ps.default_config(rank=r, world=2, cuts=[0, 7, 16], **over)) for r in range(2)]
    for s in [one] + ranks:
        s.fill_particles(xyz, age=age, fert_age=np.float32(1e6), vxyz=v)
    slab.to_pairs(ranks)
    for s in ranks:
        with pytest.raises(ps.PsamdError) as e:
            s.probe(dev4(xyz[:64]))
        assert e.value.status == ERR_UNSUPPORTED
    slab.apply_stage(ranks)
    slab.finish_stage(ranks)
    one.step(1)
    def state(systems):
        ex = [s.export_live(ps.EXPORT_ALL) for s in systems]
        ids = np.concatenate([e["id"].cpu().numpy() for e in ex])
        order = np.argsort(ids, kind="stable")
        return [ids[order]] + [np.concatenate([e[k].cpu().numpy() for e in ex])[order] for k in ("pos4", "vel4", "acc4", "cell")]
    for x, y in zip(state([one]), state(ranks)):
        assert len(x) > 0 and x.tobytes() == y.tobytes(), "the step after the refusal differs from the single context's"
    one.close()
    for s in ranks:
        s.close()


# ---- 9: refusals -------------------------------------------------------------------------------------------------------------

def test_state_and_arguments(the_cloud):
    xyz, age, w = the_cloud
    g = system(xyz, age, w)
    pos4 = dev4(xyz[:256])
    out4 = torch.zeros((256, 4), dtype=torch.float32, device=DEV)
    aux = torch.zeros(64, dtype=torch.int64, device=DEV)

    def call(expect, **kw):
        spec = ps.ProbeSpec(fields=3, max_count=256, pos4=pos4.data_ptr(), out4=out4.data_ptr())
        for k, val in kw.items():
            setattr(spec, k, val)
        rc = g.lib.psamd_probe(g.h, C.byref(spec))
        assert rc == expect, (kw, rc)
    call(ERR_STATE)                                              # before build_grid
    open_frame(g)
    for bad in (dict(fields=0), dict(fields=4), dict(fields=7), dict(reserved=1), dict(max_count=-1), dict(max_count=1 << 31),
                dict(pos4=None), dict(out4=None), dict(pos4=pos4.data_ptr() + 4), dict(out4=out4.data_ptr() + 8),
                dict(outcome_dev=aux.data_ptr() + 2), dict(count_dev=aux.data_ptr() + 4), dict(result_dev=aux.data_ptr() + 4)):
        call(ERR_INVALID_ARG, **bad)
    assert g.lib.psamd_probe(g.h, None) == ERR_INVALID_ARG
    call(0)
    call(0, max_count=0, pos4=None, out4=None)                   # nothing to read or write
    g.synchronize()
    # a capture that needs growth is refused; the same capture after the growth is not
    big_in, big_out = torch.zeros((50000, 4), dtype=torch.float32, device=DEV), torch.zeros((50000, 4), dtype=torch.float32, device=DEV)
    spec = ps.ProbeSpec(fields=3, max_count=50000, pos4=big_in.data_ptr(), out4=big_out.data_ptr())
    with captured(g) as cap:
        rc = g.lib.psamd_probe(g.h, C.byref(spec))
    assert rc == ERR_STATE
    cap.close()
    call(0)                                                      # the context stays usable
    # a probe between two stage calls leaves the step's bytes unchanged
    h = system(xyz, age, w)
    open_frame(h)
    g.calc_forces_pairs(); h.calc_forces_pairs()
    g.probe(pos4)
    g.calc_forces_apply(); h.calc_forces_apply()
    assert g.download_particles().tobytes() == h.download_particles().tobytes()
    call(ERR_STATE)                                              # after calc_forces
    open_frame(g)
    call(0)
    g.inject(dev4(np.array([(1.0, 2.0, 3.0)], np.float32)))
    call(ERR_STATE)                                              # an inject ends the frame
    g.synchronize()
    g.close(); h.close()
