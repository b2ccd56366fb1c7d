"""PSAMD_FLAG_FAR_PYRAMID on the device (include/psamd.h, "a pyramid of monopoles"): the moments of every level bit for bit
against the numpy model (far_pyramid_model.py), the force records against the model's fp64 sums (1e-5 relative, the project's
bar for sums of this kind), the two exact limits (G <= 4: the far-monopole context's bytes; no far cell: the cutoff context's),
lanes of one wave under different parents, fast math, determinism and the refusals.

The small contexts hold max_particles_num=16384; the grids are 4^3 (one level), 6^3 (levels 6, 3), 8^3 (8, 4), 10^3 (10, 5, 3:
an odd level with a ragged parent) and 16^3 (16, 8, 4)."""
import ctypes

import numpy as np
import pytest

import far_monopole_model as M
import far_pyramid_model as Y
import particlesystem_amd as ps
from util import assert_same_particles, cloud

pytestmark = pytest.mark.gpu

PYR, MONO = ps.FLAG_FAR_PYRAMID, ps.FLAG_FAR_MONOPOLE
GRID = {4: dict(max_particles_num=16384, chunk_factor=1, chunk_dim=4),
        6: dict(max_particles_num=16384, chunk_factor=2, chunk_dim=3),
        8: dict(max_particles_num=16384, chunk_factor=2, chunk_dim=4),
        10: dict(max_particles_num=16384, chunk_factor=2, chunk_dim=5),
        16: dict(max_particles_num=16384, chunk_factor=4, chunk_dim=4, x_factor=8)}      # (x_factor: lists of 40, for 4 a cell in the mean)
REL = 1e-5
INVALID_ARG, STATE, UNSUPPORTED = 1, 8, 9


def frame(g, apply=True, slab=False):
    """one frame up to the pair stage: (slot ids in sorted order, force records, cell lists as slot ids, the levels' moments
    on a pyramid context or None)"""
    if slab:
        g.slab_build(); g.slab_pairs()
    else:
        g.init_iframe(); g.build_grid(); g.calc_forces_pairs()
    rows = g.download_cellgrid()
    lists = [row[1:1 + row[0]] for row in rows]
    order = np.concatenate(lists)
    f = g.download_force4(0, len(order))
    mom = [g.download_level_moments(l) for l in range(len(ps.far_levels(g.cfg)))] if g.cfg.flags & PYR else None
    if apply:
        if slab:
            g.slab_apply(); g.slab_finish()
        else:
            g.calc_forces_apply()
    return order, f, lists, mom


def index_of(g, ids):
    """slot id -> index into the arrays the fill was given"""
    where = np.full(g.sizes.container_size, -1, np.int64)
    where[ids] = np.arange(len(ids))
    return where


def box_cloud(n, seed, G):
    return cloud(n, seed, G * 2.5 * 0.9995)


def low_corner(i1, i2, i3, G):
    """of a cell (i2 ~ +x, i1 ~ -y, i3 ~ -z)"""
    return np.array([(i2 - G // 2) * 5.0, -(i1 - G // 2) * 5.0 - 5.0, -(i3 - G // 2) * 5.0 - 5.0])


# ---- 1. moments -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("G", [8, 10])
def test_moments_of_every_level_equal_the_model_bit_for_bit(G, sign):
    """kids among the adults, unequal masses, one cell of kids only; on 8^3 one cell with more particles than its list holds
    (only the first MAX_PARTICLES_PER_CELL count; the list is longer than 64, so the sum takes a second round of lanes).
    10^3: level 1 has 5 cells an axis, so level 2's last parents have one child an axis"""
    g = ps.ParticleSystem(ps.default_config(flags=PYR, force_sign=sign, collision_radius=1e-6, **GRID[G]))
    assert g.sizes.grid_dim == G
    cap = g.sizes.max_per_cell
    rng = np.random.default_rng(21)
    xyz = box_cloud(12 * G ** 3, 21, G)
    cell = M.cells_of(xyz, G)
    full, kids_only = (3 * G + 4) * G + 2, (5 * G + 1) * G + 6
    xyz = xyz[(cell != full) & (cell != kids_only)]
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
    g.init_iframe(); g.build_grid(); g.calc_forces_pairs()
    lists = [row[1:1 + row[0]] for row in g.download_cellgrid()]
    mom = [g.download_level_moments(l) for l in range(len(Y.levels_of(G)))]
    cells = g.download_cell_moments()
    g.calc_forces_apply()
    where = index_of(g, ids)
    lists = [where[l] for l in lists]
    if G == 8:
        assert cap > 64 and len(lists[full]) == cap and g.counters["cell_overflow_kills"] >= 14
    w_eff = np.where(age < 1.5, np.float32(0.0), np.float32(sign) * w).astype(np.float32)
    want = Y.level_moments(lists, xyz, w_eff, G)
    assert np.array_equal(want[0], M.moments(lists, xyz, w_eff)) and cells.tobytes() == mom[0].tobytes()
    assert not want[0][kids_only].any() and want[0][full, 3] != 0
    for l, (got, exp) in enumerate(zip(mom, want)):
        assert got.shape == exp.shape == (Y.levels_of(G)[l] ** 3, 4)
        bad = np.nonzero((got.view(np.uint32) != exp.view(np.uint32)).any(1))[0]
        assert len(bad) == 0, ("level %d: moments differ from the model in %d cells, first %d: device %r model %r"
                               % (l, len(bad), bad[0], got[bad[0]], exp[bad[0]]))
        assert (exp[:, 3] != 0).all() or l == 0
        assert ((exp[:, 3] > 0) == (sign > 0))[exp[:, 3] != 0].all()
    g.close()


# ---- 2. the two exact limits ------------------------------------------------------------------------------------------------

def lively(n, seed, G):
    rng = np.random.default_rng(seed)
    age = rng.uniform(0.2, 9.0, n).astype(np.float32)
    return dict(xyz=box_cloud(n, seed, G), age=age, w=rng.uniform(20.0, 100.0, n).astype(np.float32),
                fert_age=rng.uniform(3.0, 12.0, n).astype(np.float32), vxyz=rng.uniform(-8, 8, (n, 3)).astype(np.float32))


def test_one_level_is_the_far_monopole_context_byte_for_byte():
    """G = 4: one level, one block of 64 cells -- the records of a frame and three whole steps (births on) are those of a
    PSAMD_FLAG_FAR_MONOPOLE context given the same fill: its 15 empty parts add +0"""
    c = lively(2048, 81, 4)
    out = []
    for flag in (PYR, MONO):
        g = ps.ParticleSystem(ps.default_config(flags=flag | ps.FLAG_EXPLOSIONS, **GRID[4]))
        assert g.sizes.grid_dim == 4
        g.fill_particles(**c)
        g.snapshot_save()
        order, f, _, _ = frame(g)
        g.snapshot_restore()
        g.step(3)
        out.append((order, f, g.download_particles(), g.counters))
        g.close()
    (oa, fa, pa, ca), (ob, fb, pb, cb) = out
    assert np.array_equal(oa, ob) and np.abs(fa[:, :3]).max() > 0 and fa.tobytes() == fb.tobytes()
    assert_same_particles(pa, pb, "three steps on 4^3 cells, pyramid against far monopoles")
    assert ca == cb and ca["integrated"] > 3000 and ca["births"] > 0


def test_confined_cloud_is_the_cutoff_result_byte_for_byte():
    """a cloud inside a 2x2x2 block of cells of the default 16^3 grid (cells 7..8 on every axis: two parents at every level):
    no ancestor of a stencil cell is in the set -- the records and the whole step are the cutoff context's"""
    n = 3000
    rng = np.random.default_rng(7)
    xyz = rng.uniform(-4.99, 4.99, (n, 3)).astype(np.float32)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    a = ps.ParticleSystem(ps.default_config(flags=PYR))
    b = ps.ParticleSystem(ps.default_config())
    for s in (a, b):
        s.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    oa, fa, _, mom = frame(a)
    ob, fb, _, _ = frame(b)
    assert np.array_equal(oa, ob) and np.abs(fa[:, :3]).max() > 0 and fa.tobytes() == fb.tobytes()
    assert [int((m[:, 3] != 0).sum()) for m in mom] == [8, 8, 8]
    assert_same_particles(a.download_particles(), b.download_particles(), "pyramid step on a confined cloud")
    a.close(); b.close()


# ---- 3. against the model ---------------------------------------------------------------------------------------------------

def model_frame(G, flags, seed, n):
    """a uniform cloud of n bodies, some of them kids, one frame: (records in sorted order, their index into the fill, the
    lists as indices into the fill, positions, w_eff, kid mask)"""
    g = ps.ParticleSystem(ps.default_config(flags=flags, collision_radius=1e-6, **GRID[G]))
    assert g.sizes.grid_dim == G
    xyz = box_cloud(n, seed, G)
    rng = np.random.default_rng(seed)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    age[::17] = 0.5                                                       # some kids: exert and feel nothing
    ids = g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    order, f, lists, _ = frame(g)
    where = index_of(g, ids)
    assert len(order) == n and g.counters["cell_overflow_kills"] == 0
    g.close()
    kid = age < 1.5
    w_eff = np.where(kid, np.float32(0.0), np.float32(60.0)).astype(np.float32)
    return f, where[order], [where[l] for l in lists], xyz, w_eff, kid


def against_the_model(G, flags, seed, n):
    f, idx, lists, xyz, w_eff, kid = model_frame(G, flags, seed, n)
    adults = np.nonzero(~kid[idx])[0]
    want = Y.accel(lists, xyz, w_eff, G, 0.2, idx[adults])
    got = f[:, :3].astype(np.float64)
    rel = M.rel_dev(got[adults], want)
    cutoff = M.rel_dev(Y.accel(lists, xyz, w_eff, G, 0.2, idx[adults], far=False), want)
    print("pyramid, %d bodies on %d^3 cells, flags %#x: max relative deviation from the model %.3g (the stencil alone: median %.3g)"
          % (n, G, flags, rel.max(), np.median(cutoff)))
    assert (f[:, 3].view(np.int32) == 0).all() and not got[kid[idx]].any()
    assert np.median(cutoff) > 0.1                                       # (the far part is no small correction here)
    return rel, f


@pytest.mark.parametrize("G,per_cell", [(6, 16), (8, 16), (10, 16), (16, 4)], ids=["6^3", "8^3", "10^3", "16^3"])
def test_force_records_follow_the_model(G, per_cell):
    """6^3: levels 6, 3; 8^3: 8, 4; 10^3: 10, 5, 3 with ragged parents; 16^3: three levels, 64 blocks at level 0, of which a
    wave walks a few.  At about 16 bodies a cell (16^3: 4, 16384 bodies) the reference's own serial chain over the stencil
    meets the project's bar for a whole sum (test_gpu_far_monopole.py explains), so it can be asked of the record.
    Measured on an MI355X: 6^3 2.3e-6, 8^3 4.3e-6, 10^3 2.1e-6, 16^3 1.1e-6"""
    rel, _ = against_the_model(G, PYR, 30 + G, per_cell * G ** 3)
    assert rel.max() < REL


def test_the_far_part_alone_on_dense_cells():
    """16384 bodies on 8^3 cells, 32 a cell: what the walk and the combine ADD to the stencil's chain -- the record of a
    pyramid context minus the record of a cutoff context on the same cloud -- against the model's far part, on the scale of
    the particle's whole |a|, so that a wrong mask cannot hide behind a large stencil sum (measured: 1.8e-6)"""
    G, n = 8, 16384
    f, idx, lists, xyz, w_eff, kid = model_frame(G, PYR, 34, n)
    f0, idx0, _, _, _, _ = model_frame(G, 0, 34, n)
    assert np.array_equal(idx, idx0) and (f[:, 3].view(np.int32) == 0).all()
    adults = np.nonzero(~kid[idx])[0]
    near = Y.accel(lists, xyz, w_eff, G, 0.2, idx[adults], far=False)
    whole = Y.accel(lists, xyz, w_eff, G, 0.2, idx[adults])
    far = whole - near
    got = f[adults, :3].astype(np.float64) - f0[adults, :3].astype(np.float64)
    rel = np.linalg.norm(got - far, axis=1) / np.linalg.norm(whole, axis=1)
    print("far part alone, %d bodies on %d^3 cells: max deviation from the model's far part over |a| %.3g" % (n, G, rel.max()))
    assert np.abs(far).max() > 0 and rel.max() < REL


def test_lanes_of_one_wave_under_different_parents():
    """700 bodies on 8^3 cells, one or two a cell: the 64 served particles of a wave come from some 50 cells, which lie under
    several parents at either level -- every lane masks by its own parent (measured: 7.2e-7)"""
    G, n = 8, 700
    f, idx, lists, xyz, w_eff, kid = model_frame(G, PYR, 35, n)
    cells = M.cells_of(xyz[idx], G)
    assert (np.diff(cells) >= 0).all()                                   # (sorted order: the dense tasks take the served ones in it)
    i1, i2, i3 = (cells // G % G) >> 1, (cells % G) >> 1, (cells // (G * G)) >> 1
    assert len(np.unique(((i3 * 4 + i1) * 4 + i2)[:64])) >= 8            # one wave's worth of particles, many parents
    adults = np.nonzero(~kid[idx])[0]
    want = Y.accel(lists, xyz, w_eff, G, 0.2, idx[adults])
    rel = M.rel_dev(f[adults, :3].astype(np.float64), want)
    print("sparse cloud, %d bodies on %d^3 cells: max relative deviation from the model %.3g" % (n, G, rel.max()))
    assert (f[:, 3].view(np.int32) == 0).all() and rel.max() < REL


# ---- 4. fast math -----------------------------------------------------------------------------------------------------------

def test_fast_math_follows_the_model_and_gives_the_same_bytes_twice():
    rel, f1 = against_the_model(8, PYR | ps.FLAG_FAST_MATH, 51, 8192)
    assert rel.max() < REL                                            # the tolerance mode's bar for uniform clouds (test_gpu_fast.py)
    _, f2 = against_the_model(8, PYR | ps.FLAG_FAST_MATH, 51, 8192)
    assert f1.tobytes() == f2.tobytes()


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------

def test_the_same_frame_gives_the_same_records_however_it_is_run():
    """plain stage calls; the slab family's calls with graphs on (captured, then replayed); run-ahead 0; after two steps
    and a snapshot_restore"""
    c = lively(8192, 61, 8)

    def records(graphs=False, run_ahead=1, detour=False):
        g = ps.ParticleSystem(ps.default_config(flags=PYR, **GRID[8]))
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
        order, f, _, mom = frame(g, slab=graphs)
        if graphs:
            assert g.graph_stats()[0] > 0
        g.close()
        return order.tobytes(), f.tobytes(), b"".join(m.tobytes() for m in mom)

    base = records()
    assert np.abs(np.frombuffer(base[1], np.float32)).max() > 0
    assert records(graphs=True) == base, "graphs on"
    assert records(run_ahead=0) == base, "run-ahead 0"
    assert records(detour=True) == base, "after snapshot_restore"


def test_three_steps_with_explosions_graphs_on_and_off():
    c = lively(8192, 62, 8)
    out = []
    for graphs in (False, True):
        g = ps.ParticleSystem(ps.default_config(flags=PYR | ps.FLAG_EXPLOSIONS, **GRID[8]))
        g.fill_particles(**c)
        if graphs:
            g.set_graphs(True)
        g.step(3)
        out.append((g.download_particles(), g.counters))
        if graphs:
            assert g.graph_stats()[0] > 0
        g.close()
    assert_same_particles(out[1][0], out[0][0], "three pyramid steps with explosions, graphs on against off")
    assert out[0][1] == out[1][1] and out[0][1]["integrated"] > 5000


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------

def status_of_create(**over):
    with pytest.raises(ps.PsamdError) as e:
        ps.ParticleSystem(ps.default_config(**over))
    return e.value.status


def test_refusals():
    assert status_of_create(flags=PYR | ps.FLAG_ALL_PAIRS) == INVALID_ARG
    assert status_of_create(flags=PYR | MONO) == INVALID_ARG
    assert status_of_create(flags=PYR, world=2, rank=0) == UNSUPPORTED
    assert status_of_create(flags=PYR, eps2=1e-8) == UNSUPPORTED         # (eps2^3 below 2^-60: outside the lean range)
    assert status_of_create(flags=PYR, collision_radius=4.0) == UNSUPPORTED      # (no two-pass pair stage)
    g = ps.ParticleSystem(ps.default_config(flags=PYR, **GRID[8]))
    g.fill_particles(box_cloud(2000, 71, 8), age=np.float32(3.0), fert_age=np.float32(1e6))
    g.init_iframe(); g.build_grid()
    out = np.zeros((g.sizes.num_cells, 4), np.float32)
    vp = out.ctypes.data_as(ctypes.c_void_p)
    assert g.lib.psamd_download_level_moments(g.h, 0, vp) == STATE       # before the pair stage
    assert g.lib.psamd_download_cell_moments(g.h, vp) == STATE
    assert g.lib.psamd_potential(g.h, ctypes.byref(ps.Potential())) == UNSUPPORTED
    assert g.lib.psamd_download_potential(g.h, None, 0, None) == UNSUPPORTED
    assert g.lib.psamd_probe(g.h, ctypes.byref(ps.ProbeSpec(fields=ps.PROBE_ACC, max_count=0))) == UNSUPPORTED
    g.calc_forces_pairs()
    assert g.lib.psamd_download_level_moments(g.h, -1, vp) == INVALID_ARG
    assert g.lib.psamd_download_level_moments(g.h, 2, vp) == INVALID_ARG    # (levels 8, 4: L = 1)
    assert (g.download_level_moments(1)[:, 3] != 0).all()
    g.calc_forces_apply()
    assert g.lib.psamd_download_level_moments(g.h, 0, vp) == STATE       # the frame has ended
    g.step(1); g.synchronize()                                            # the context stayed usable
    assert g.counters["integrated"] >= 3900 and g.live_count() >= 1950
    g.close()
    for flags in (0, MONO):
        b = ps.ParticleSystem(ps.default_config(flags=flags, **GRID[8]))
        b.fill_particles(box_cloud(2000, 71, 8), age=np.float32(3.0), fert_age=np.float32(1e6))
        b.init_iframe(); b.build_grid(); b.calc_forces_pairs()
        assert b.lib.psamd_download_level_moments(b.h, 0, vp) == UNSUPPORTED
        b.calc_forces_apply()
        b.close()
