"""PSAMD_FLAG_FAR_QUADRUPOLE on the device (include/psamd.h, "quadrupoles on the pyramid"): the ten moment planes of every
level bit for bit against the numpy model (far_quadrupole_model.py), the two exact limits (G <= 4 with at most one adult per
cell: the pyramid context's bytes; no far cell: the cutoff context's), the force records against the model's fp64 sums
(1e-5 relative, the project's bar for sums of this kind), the quadrupole part alone, the gain in accuracy on the device,
lanes of one wave under different parents, fast math, determinism and the refusals.

The small contexts and grids are test_gpu_far_pyramid.py's (max_particles_num=16384; 4^3, 6^3, 8^3, 10^3, 16^3 cells)."""
import ctypes

import numpy as np
import pytest

import far_monopole_model as M
import far_pyramid_model as Y
import far_quadrupole_model as Q
import particlesystem_amd as ps
from test_gpu_far_pyramid import GRID, box_cloud, index_of, lively, low_corner, status_of_create
from util import assert_same_particles, cloud

pytestmark = pytest.mark.gpu

PYR = ps.FLAG_FAR_PYRAMID
QUAD = ps.FLAG_FAR_PYRAMID | ps.FLAG_FAR_QUADRUPOLE
REL = 1e-5
INVALID_ARG, STATE, UNSUPPORTED = 1, 8, 9


def frame(g, apply=True, slab=False):
    """one frame up to the pair stage: (slot ids in sorted order, force records, cell lists as slot ids, the levels' (X, Y, Z,
    M) on a pyramid context or None, the levels' six C planes on a quadrupole context or None)"""
    if slab:
        g.slab_build(); g.slab_pairs()
    else:
        g.init_iframe(); g.build_grid(); g.calc_forces_pairs()
    rows = g.download_cellgrid()
    lists = [row[1:1 + row[0]] for row in rows]
    order = np.concatenate(lists)
    f = g.download_force4(0, len(order))
    levels = range(len(ps.far_levels(g.cfg)))
    mom = [g.download_level_moments(l) for l in levels] if g.cfg.flags & PYR else None
    cen = [g.download_level_quadrupoles(l) for l in levels] if g.cfg.flags & ps.FLAG_FAR_QUADRUPOLE else None
    if apply:
        if slab:
            g.slab_apply(); g.slab_finish()
        else:
            g.calc_forces_apply()
    return order, f, lists, mom, cen


# ---- 1. moments -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("G", [8, 10])
def test_moments_of_every_level_equal_the_model_bit_for_bit(G, sign):
    """the cloud of test_gpu_far_pyramid.py's test of this name: kids among the adults, unequal masses, one cell of kids only
    (its C is all zeros); on 8^3 one cell with more entries than its list holds and more than 64 (the sums take a second round
    of lanes).  X, Y, Z and M are a plain pyramid context's bytes"""
    rng = np.random.default_rng(21)
    xyz = box_cloud(12 * G ** 3, 21, G)
    cell = M.cells_of(xyz, G)
    full, kids_only = (3 * G + 4) * G + 2, (5 * G + 1) * G + 6
    xyz = xyz[(cell != full) & (cell != kids_only)]
    got = {}
    for flags in (QUAD, PYR):
        g = ps.ParticleSystem(ps.default_config(flags=flags, force_sign=sign, collision_radius=1e-6, **GRID[G]))
        assert g.sizes.grid_dim == G
        cap = g.sizes.max_per_cell
        if flags == QUAD:
            n_crowd = cap + 14 if G == 8 else 20
            crowd = (low_corner(4, 2, 3, G) + rng.uniform(0.05, 4.95, (n_crowd, 3))).astype(np.float32)
            nursery = (low_corner(1, 6, 5, G) + rng.uniform(0.05, 4.95, (5, 3))).astype(np.float32)
            age = rng.uniform(15 / 7, 7.5, len(xyz)).astype(np.float32)
            age[::13] = 0.5
            xyz = np.concatenate([xyz, crowd, nursery])
            age = np.concatenate([age, np.full(len(crowd), 3.0, np.float32), np.full(5, 0.5, np.float32)])
            assert (M.cells_of(crowd, G) == full).all() and (M.cells_of(nursery, G) == kids_only).all()
            w = rng.uniform(20.0, 100.0, len(xyz)).astype(np.float32)
        ids = g.fill_particles(xyz, age=age, w=w, fert_age=np.float32(1e6))
        _, _, lists, mom, cen = frame(g)
        if G == 8:
            assert cap > 64 and len(lists[full]) == cap and g.counters["cell_overflow_kills"] >= 14
        got[flags] = (index_of(g, ids), lists, mom, cen)
        g.close()
    where, lists, mom, cen = got[QUAD]
    assert got[PYR][3] is None and b"".join(m.tobytes() for m in mom) == b"".join(m.tobytes() for m in got[PYR][2])
    lists = [where[l] for l in lists]
    w_eff = np.where(age < 1.5, np.float32(0.0), np.float32(sign) * w).astype(np.float32)
    want_mom, want_cen = Q.level_moments(lists, xyz, w_eff, G)
    assert not want_cen[0][kids_only].any() and want_cen[0][full].all() and len(mom) == len(want_mom) == len(Y.levels_of(G))
    for l in range(len(mom)):
        assert mom[l].tobytes() == want_mom[l].tobytes(), "level %d: X, Y, Z, M differ from the model" % l
        assert cen[l].shape == want_cen[l].shape == (Y.levels_of(G)[l] ** 3, 6)
        bad = np.nonzero((cen[l].view(np.uint32) != want_cen[l].view(np.uint32)).any(1))[0]
        assert len(bad) == 0, ("level %d: second moments differ from the model in %d cells, first %d: device %r model %r"
                               % (l, len(bad), bad[0], cen[l][bad[0]], want_cen[l][bad[0]]))
        diag = want_cen[l][:, :3]
        assert (np.sign(diag[diag != 0]) == sign).all() and (diag != 0).any()      # (Caa has M's sign)


# ---- 2. the two exact limits ------------------------------------------------------------------------------------------------

def test_one_adult_per_cell_on_one_level_is_the_pyramid_context_byte_for_byte():
    """4^3 cells (one level): an adult in 56 of the 64 cells and 300 kids anywhere -- every C is an exact zero and every
    quadrupole chain +0, so the records of a frame and three whole steps are the PSAMD_FLAG_FAR_PYRAMID context's.  The
    adults start at rest near their cells' centres and three steps move them by little: the last frame's C planes, all
    zeros, show that the condition held to the end"""
    G = 4
    rng = np.random.default_rng(82)
    cells = rng.permutation(G ** 3)[:56]
    corner = np.array([low_corner(c // G % G, c % G, c // (G * G), G) for c in cells])
    adults = (corner + rng.uniform(2.0, 3.0, (56, 3))).astype(np.float32)
    assert sorted(M.cells_of(adults, G).tolist()) == sorted(cells.tolist())
    kids = box_cloud(300, 83, G)
    fill = dict(xyz=np.concatenate([adults, kids]), w=rng.uniform(20.0, 100.0, 356).astype(np.float32), fert_age=np.float32(1e6),
                age=np.concatenate([rng.uniform(15 / 7, 7.5, 56), np.full(300, 0.25)]).astype(np.float32),
                vxyz=np.concatenate([np.zeros((56, 3)), rng.uniform(-8, 8, (300, 3))]).astype(np.float32))
    out = []
    for flags in (QUAD, PYR):
        g = ps.ParticleSystem(ps.default_config(flags=flags, **GRID[G]))
        assert g.sizes.grid_dim == G
        g.fill_particles(**fill)
        g.snapshot_save()
        order, f, _, mom, cen = frame(g)
        g.snapshot_restore()
        g.step(3)
        last = frame(g)
        out.append((order, f, g.download_particles(), g.counters, mom, cen, last))
        g.close()
    (oa, fa, pa, ca, ma, qa, la), (ob, fb, pb, cb, mb, _, lb) = out
    assert np.array_equal(oa, ob) and np.abs(fa[:, :3]).max() > 0 and fa.tobytes() == fb.tobytes()
    assert ma[0].tobytes() == mb[0].tobytes() and int((ma[0][:, 3] != 0).sum()) == 56
    assert qa[0].tobytes() == bytes(24 * G ** 3) and la[4][0].tobytes() == bytes(24 * G ** 3)
    assert la[1].tobytes() == lb[1].tobytes() and int((la[3][0][:, 3] != 0).sum()) == 56
    assert_same_particles(pa, pb, "three steps on 4^3 cells, one adult a cell: quadrupoles against the pyramid")
    assert ca == cb and ca["integrated"] >= 3 * 56


def test_confined_cloud_is_the_cutoff_result_byte_for_byte():
    """a cloud inside a 2x2x2 block of cells of the default 16^3 grid: no member at any level -- the records and the whole
    step are the cutoff context's, whatever the C planes hold"""
    n = 3000
    rng = np.random.default_rng(7)
    xyz = rng.uniform(-4.99, 4.99, (n, 3)).astype(np.float32)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    a = ps.ParticleSystem(ps.default_config(flags=QUAD))
    b = ps.ParticleSystem(ps.default_config())
    for s in (a, b):
        s.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    oa, fa, _, mom, cen = frame(a)
    ob, fb, _, _, _ = frame(b)
    assert np.array_equal(oa, ob) and np.abs(fa[:, :3]).max() > 0 and fa.tobytes() == fb.tobytes()
    assert [int((m[:, 3] != 0).sum()) for m in mom] == [8, 8, 8] and [int(c[:, :3].all(1).sum()) for c in cen] == [8, 8, 8]
    assert_same_particles(a.download_particles(), b.download_particles(), "quadrupole step on a confined cloud")
    a.close(); b.close()


# ---- 3. against the model ---------------------------------------------------------------------------------------------------

def model_frame(G, flags, seed, n, xyz=None, kids=True):
    """a uniform cloud of n bodies (or `xyz`), some of them kids, one frame: (records in sorted order, their index into the
    fill, the lists as indices into the fill, positions, w_eff, kid mask)"""
    g = ps.ParticleSystem(ps.default_config(flags=flags, collision_radius=1e-6, **GRID[G]))
    assert g.sizes.grid_dim == G
    if xyz is None:
        xyz = box_cloud(n, seed, G)
    rng = np.random.default_rng(seed)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    if kids:
        age[::17] = 0.5                                                   # some kids: exert and feel nothing
    ids = g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    order, f, lists, _, _ = frame(g)
    where = index_of(g, ids)
    assert len(order) == n and g.counters["cell_overflow_kills"] == 0
    g.close()
    kid = age < 1.5
    w_eff = np.where(kid, np.float32(0.0), np.float32(60.0)).astype(np.float32)
    return f, where[order], [where[l] for l in lists], xyz, w_eff, kid


def against_the_model(G, flags, seed, n):
    f, idx, lists, xyz, w_eff, kid = model_frame(G, flags, seed, n)
    adults = np.nonzero(~kid[idx])[0]
    moments = Q.level_moments(lists, xyz, w_eff, G)
    part = Q.quad_accel(lists, xyz, w_eff, G, 0.2, idx[adults], moments)
    want = Y.accel(lists, xyz, w_eff, G, 0.2, idx[adults], levmom=moments[0]) + part
    got = f[:, :3].astype(np.float64)
    rel = M.rel_dev(got[adults], want)
    share = np.linalg.norm(part, axis=1) / np.linalg.norm(want, axis=1)
    print("quadrupoles, %d bodies on %d^3 cells, flags %#x: max relative deviation from the model %.3g (the quadrupole part: "
          "median %.3g of |a|)" % (n, G, flags, rel.max(), np.median(share)))
    assert (f[:, 3].view(np.int32) == 0).all() and not got[kid[idx]].any()
    assert np.median(share) > 1e-4                                       # (the part is there to be got wrong)
    return rel, f


@pytest.mark.parametrize("G,per_cell", [(6, 16), (8, 16), (10, 16), (16, 4)], ids=["6^3", "8^3", "10^3", "16^3"])
def test_force_records_follow_the_model(G, per_cell):
    """the grids and clouds of test_gpu_far_pyramid.py's test of this name.  Measured on an MI355X: 6^3 2.2e-6, 8^3 4.2e-6, 10^3 2.0e-6, 16^3 1.2e-6 (the quadrupole part: 0.2-0.5 % of |a| for the median particle)"""
    rel, _ = against_the_model(G, QUAD, 30 + G, per_cell * G ** 3)
    assert rel.max() < REL


def test_the_quadrupole_part_alone():
    """16384 bodies on 8^3 cells: what the flag ADDS -- the record of a quadrupole context minus the record of a pyramid
    context on the same cloud -- against the model's quadrupole part, for the adults whose model part is at least 1e-3 of
    their |a| (78 % of them with this seed; at least a quarter is the condition), relative to |a_q|.  The floor is the fp32
    rounding of two records, a few 2^-23 |a|: about 3e-4 of such an a_q, so 1e-2 leaves some 30x of room, while a wrong
    coefficient or a swapped plane moves a_q by tens of percent.  Measured on an MI355X: 1.4e-4"""
    G, n = 8, 16384
    f, idx, lists, xyz, w_eff, kid = model_frame(G, QUAD, 34, n)
    f0, idx0, _, _, _, _ = model_frame(G, PYR, 34, n)
    assert np.array_equal(idx, idx0) and (f[:, 3].view(np.int32) == 0).all()
    adults = np.nonzero(~kid[idx])[0]
    moments = Q.level_moments(lists, xyz, w_eff, G)
    part = Q.quad_accel(lists, xyz, w_eff, G, 0.2, idx[adults], moments)
    whole = Y.accel(lists, xyz, w_eff, G, 0.2, idx[adults], levmom=moments[0]) + part
    size = np.linalg.norm(part, axis=1)
    use = size >= 1e-3 * np.linalg.norm(whole, axis=1)
    got = f[adults, :3].astype(np.float64) - f0[adults, :3].astype(np.float64)
    rel = np.linalg.norm(got - part, axis=1)[use] / size[use]
    print("quadrupole part alone, %d bodies on %d^3 cells: %.0f %% of the adults qualify, max deviation over |a_q| %.3g"
          % (n, G, 100 * use.mean(), rel.max()))
    assert use.mean() >= 0.25
    assert rel.max() < 1e-2


def test_the_device_is_closer_to_the_direct_sum_with_quadrupoles():
    """8192 bodies on 8^3 cells (test_far_pyramid_cpu.py's uniform cloud, seed 11), 400 sampled, against the fp64 direct sum
    over all bodies: the quadrupole context's median deviation is at most half of the pyramid context's.  Measured on an
    MI355X: median 8.35e-4 against 2.39e-3, a ratio of 0.35 (the maxima: 1.38e-2 against 4.36e-2)"""
    G, n = 8, 8192
    xyz = cloud(n, 11, G * 2.5 * 0.9995)
    pick = np.random.default_rng(13).choice(n, 400, replace=False)
    med = {}
    for flags in (QUAD, PYR):
        f, idx, _, _, w_eff, kid = model_frame(G, flags, 11, n, xyz=xyz, kids=False)
        assert not kid.any()
        got = np.empty((n, 3))
        got[idx] = f[:, :3].astype(np.float64)
        dev = M.rel_dev(got[pick], M.direct(xyz, w_eff, 0.2, pick))
        med[flags] = np.median(dev)
        print("flags %#x, %d bodies on %d^3 cells against the direct sum: median %.3g max %.3g" % (flags, n, G, med[flags], dev.max()))
    assert med[QUAD] <= 0.5 * med[PYR]


def test_lanes_of_one_wave_under_different_parents():
    """700 bodies on 8^3 cells, one or two a cell: a wave's 64 particles lie under several parents at either level, and each
    lane's members -- of both chains -- are its own.  Measured on an MI355X: 7.1e-7"""
    G, n = 8, 700
    f, idx, lists, xyz, w_eff, kid = model_frame(G, QUAD, 35, n)
    cells = M.cells_of(xyz[idx], G)
    i1, i2, i3 = (cells // G % G) >> 1, (cells % G) >> 1, (cells // (G * G)) >> 1
    assert (np.diff(cells) >= 0).all() and len(np.unique(((i3 * 4 + i1) * 4 + i2)[:64])) >= 8
    adults = np.nonzero(~kid[idx])[0]
    want = Q.accel(lists, xyz, w_eff, G, 0.2, idx[adults])
    rel = M.rel_dev(f[adults, :3].astype(np.float64), want)
    print("sparse cloud, %d bodies on %d^3 cells: max relative deviation from the model %.3g" % (n, G, rel.max()))
    assert (f[:, 3].view(np.int32) == 0).all() and rel.max() < REL


# ---- 4. fast math -----------------------------------------------------------------------------------------------------------

def test_fast_math_follows_the_model_and_gives_the_same_bytes_twice():
    """Measured on an MI355X: 3.1e-6"""
    rel, f1 = against_the_model(8, QUAD | ps.FLAG_FAST_MATH, 51, 8192)
    assert rel.max() < REL
    _, f2 = against_the_model(8, QUAD | ps.FLAG_FAST_MATH, 51, 8192)
    assert f1.tobytes() == f2.tobytes()


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------

def test_the_same_frame_gives_the_same_records_however_it_is_run():
    """plain stage calls; the slab family's calls with graphs on (captured, then replayed); run-ahead 0; after two steps
    and a snapshot_restore -- the records and all ten planes of every level"""
    c = lively(8192, 61, 8)

    def records(graphs=False, run_ahead=1, detour=False):
        g = ps.ParticleSystem(ps.default_config(flags=QUAD, **GRID[8]))
        g.fill_particles(**c)
        g.set_run_ahead(run_ahead)
        if graphs:
            g.set_graphs(True)
        if graphs or detour:
            g.snapshot_save()
            if graphs:
                frame(g, slab=True)                                   # (captures the stage sequences)
            g.step(2)
            g.snapshot_restore()
        order, f, _, mom, cen = frame(g, slab=graphs)
        if graphs:
            assert g.graph_stats()[0] > 0
        g.close()
        return order.tobytes(), f.tobytes(), b"".join(m.tobytes() for m in mom), b"".join(m.tobytes() for m in cen)

    base = records()
    assert np.abs(np.frombuffer(base[1], np.float32)).max() > 0 and np.frombuffer(base[3], np.float32).any()
    assert records(graphs=True) == base, "graphs on"
    assert records(run_ahead=0) == base, "run-ahead 0"
    assert records(detour=True) == base, "after snapshot_restore"


def test_three_steps_with_explosions_graphs_on_and_off():
    c = lively(8192, 62, 8)
    out = []
    for graphs in (False, True):
        g = ps.ParticleSystem(ps.default_config(flags=QUAD | ps.FLAG_EXPLOSIONS, **GRID[8]))
        g.fill_particles(**c)
        if graphs:
            g.set_graphs(True)
        g.step(3)
        out.append((g.download_particles(), g.counters))
        if graphs:
            assert g.graph_stats()[0] > 0
        g.close()
    assert_same_particles(out[1][0], out[0][0], "three quadrupole steps with explosions, graphs on against off")
    assert out[0][1] == out[1][1] and out[0][1]["integrated"] > 5000


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals():
    assert status_of_create(flags=ps.FLAG_FAR_QUADRUPOLE) == INVALID_ARG      # the flag alone
    assert status_of_create(flags=ps.FLAG_FAR_QUADRUPOLE | ps.FLAG_FAR_MONOPOLE) == INVALID_ARG
    assert status_of_create(flags=QUAD | ps.FLAG_ALL_PAIRS) == INVALID_ARG
    assert status_of_create(flags=QUAD | ps.FLAG_FAR_MONOPOLE) == INVALID_ARG
    assert status_of_create(flags=QUAD, world=2, rank=0) == UNSUPPORTED
    assert status_of_create(flags=QUAD, eps2=1e-8) == UNSUPPORTED
    assert status_of_create(flags=QUAD, collision_radius=4.0) == UNSUPPORTED
    g = ps.ParticleSystem(ps.default_config(flags=QUAD, **GRID[8]))
    g.fill_particles(box_cloud(2000, 71, 8), age=np.float32(3.0), fert_age=np.float32(1e6))
    g.init_iframe(); g.build_grid()
    out = np.zeros((g.sizes.num_cells, 6), np.float32)
    vp = out.ctypes.data_as(ctypes.c_void_p)
    assert g.lib.psamd_download_level_quadrupoles(g.h, 0, vp) == STATE    # before the pair stage
    for flags in (0, ps.POTENTIAL_FAR):
        assert g.lib.psamd_potential(g.h, ctypes.byref(ps.Potential(flags=flags))) == UNSUPPORTED
    assert g.lib.psamd_download_potential(g.h, None, 0, None) == UNSUPPORTED
    assert g.lib.psamd_download_potential_far(g.h, None, 0, None) == UNSUPPORTED
    for far in (0, ps.PROBE_FAR):
        assert g.lib.psamd_probe(g.h, ctypes.byref(ps.ProbeSpec(fields=ps.PROBE_ACC | far, max_count=0))) == UNSUPPORTED
    g.calc_forces_pairs()
    assert g.lib.psamd_download_level_quadrupoles(g.h, -1, vp) == INVALID_ARG
    assert g.lib.psamd_download_level_quadrupoles(g.h, 2, vp) == INVALID_ARG      # (levels 8, 4: L = 1)
    assert g.lib.psamd_download_level_quadrupoles(g.h, 0, None) == INVALID_ARG
    assert g.download_level_quadrupoles(1)[:, :3].all()
    g.calc_forces_apply()
    assert g.lib.psamd_download_level_quadrupoles(g.h, 0, vp) == STATE    # the frame has ended
    g.step(1); g.synchronize()                                            # the context stayed usable
    assert g.counters["integrated"] >= 3900 and g.live_count() >= 1950
    g.close()
    for flags in (0, PYR):
        b = ps.ParticleSystem(ps.default_config(flags=flags, **GRID[8]))
        b.fill_particles(box_cloud(2000, 71, 8), age=np.float32(3.0), fert_age=np.float32(1e6))
        b.init_iframe(); b.build_grid(); b.calc_forces_pairs()
        assert b.lib.psamd_download_level_quadrupoles(b.h, 0, vp) == UNSUPPORTED
        b.calc_forces_apply()
        b.close()
