"""PSAMD_FLAG_FAR_MONOPOLE on the device (include/psamd.h, "long-range gravity"): the cells' moments bit for bit against
the numpy model (far_monopole_model.py), the force records against the model's fp64 sums (1e-5 relative, the project's
bar for sums of this kind), the two exact limits (no far cell: the cutoff result, byte for byte; one adult per cell:
the all-pairs force), determinism, the refusals, and once one size up against an fp64 direct sum.

The small contexts use 8^3 cells of about 16 bodies (max_particles_num=16384, chunk_factor=2, chunk_dim=4) unless noted."""
import ctypes

import numpy as np
import pytest

import far_monopole_model as M
import oracle_py as O
import particlesystem_amd as ps
from util import assert_same_particles, cloud, oracle_cfg_from

pytestmark = pytest.mark.gpu

FAR = ps.FLAG_FAR_MONOPOLE
SMALL = dict(max_particles_num=16384, chunk_factor=2, chunk_dim=4)
REL = 1e-5
INVALID_ARG, STATE, UNSUPPORTED = 1, 8, 9


def frame(g, apply=True, slab=False):
    """one frame up to the pair stage: (slot ids in sorted order, force records, cell lists as slot ids, moments or None)"""
    if slab:
        g.slab_build(); g.slab_pairs()
    else:
        g.init_iframe(); g.build_grid(); g.calc_forces_pairs()
    rows = g.download_cellgrid()
    lists = [row[1:1 + row[0]] for row in rows]
    order = np.concatenate(lists)
    f = g.download_force4(0, len(order))
    mom = g.download_cell_moments() if g.cfg.flags & FAR else None
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


# ---- 1. moments -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_moments_equal_the_model_bit_for_bit(sign):
    """kids among the adults, unequal masses, one cell of kids only, one cell with more particles than its list holds (only
    the first MAX_PARTICLES_PER_CELL count; the list is longer than 64, so the sum takes a second round of lanes)"""
    G, n = 8, 6000
    g = ps.ParticleSystem(ps.default_config(flags=FAR, force_sign=sign, collision_radius=1e-6, **SMALL))
    cap = g.sizes.max_per_cell
    assert cap > 64
    rng = np.random.default_rng(21)
    xyz = box_cloud(n, 21, G)
    cell = M.cells_of(xyz, G)
    full, kids_only = (3 * G + 4) * G + 2, (5 * G + 1) * G + 6
    xyz = xyz[(cell != full) & (cell != kids_only)]
    lo_full = np.array([(2 - G // 2) * 5.0, -(4 - G // 2) * 5.0 - 5.0, -(3 - G // 2) * 5.0 - 5.0])      # low corner of `full` (i2 ~ +x, i1 ~ -y, i3 ~ -z)
    lo_kids = np.array([(6 - G // 2) * 5.0, -(1 - G // 2) * 5.0 - 5.0, -(5 - G // 2) * 5.0 - 5.0])
    crowd = (lo_full + rng.uniform(0.05, 4.95, (cap + 14, 3))).astype(np.float32)
    nursery = (lo_kids + rng.uniform(0.05, 4.95, (5, 3))).astype(np.float32)
    age = rng.uniform(15 / 7, 7.5, len(xyz)).astype(np.float32)
    age[::13] = 0.5
    xyz = np.concatenate([xyz, crowd, nursery])
    age = np.concatenate([age, np.full(len(crowd), 3.0, np.float32), np.full(5, 0.5, np.float32)])
    assert (M.cells_of(crowd, G) == full).all() and (M.cells_of(nursery, G) == kids_only).all()
    w = rng.uniform(20.0, 100.0, len(xyz)).astype(np.float32)
    ids = g.fill_particles(xyz, age=age, w=w, fert_age=np.float32(1e6))
    order, f, lists, mom = frame(g)
    where = index_of(g, ids)
    lists = [where[l] for l in lists]
    assert len(lists[full]) == cap and g.counters["cell_overflow_kills"] >= 14
    w_eff = np.where(age < 1.5, np.float32(0.0), np.float32(sign) * w).astype(np.float32)
    want = M.moments(lists, xyz, w_eff)
    assert not want[kids_only].any() and want[full, 3] != 0 and (want[:, 3] != 0).sum() > 400
    bad = np.nonzero((mom.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    assert len(bad) == 0, "moments differ from the model in %d cells, first %d: device %r model %r" % (len(bad), bad[0], mom[bad[0]], want[bad[0]])
    assert ((want[:, 3] > 0) == (sign > 0))[want[:, 3] != 0].all()
    g.close()


# ---- 2. no far cell: the cutoff result -----------------------------------------------------------------------------------

def test_confined_cloud_is_the_cutoff_result_byte_for_byte():
    """a cloud inside a 2x2x2 block of cells: every cell of the block is in every other's stencil, no cell is far -- the
    force records and the whole step are the cutoff context's and the oracle's, byte for byte"""
    n = 3000
    rng = np.random.default_rng(7)
    xyz = rng.uniform(-4.99, 4.99, (n, 3)).astype(np.float32)           # cells 7..8 on every axis
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    a = ps.ParticleSystem(ps.default_config(flags=FAR))
    b = ps.ParticleSystem(ps.default_config())
    o = O.System(oracle_cfg_from(b.cfg))
    for s in (a, b):
        s.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    o.fill(xyz, age=age, fert_age=np.float32(1e6))
    oa, fa, _, mom = frame(a)
    ob, fb, _, _ = frame(b)
    assert np.array_equal(oa, ob) and fa.tobytes() == fb.tobytes()
    assert (mom[:, 3] != 0).sum() == 8
    o.step(1)
    assert_same_particles(a.download_particles(), o.particles, "far-monopole step on a confined cloud")
    a.close(); b.close(); o.close()


# ---- 3. against the model ---------------------------------------------------------------------------------------------------

def model_frame(over, G, flags, seed, n):
    """a uniform cloud of n bodies, some of them kids, one frame: (records in sorted order, their index into the fill, the
    lists as indices into the fill, positions, w_eff, kid mask)"""
    g = ps.ParticleSystem(ps.default_config(flags=flags, collision_radius=1e-6, **over))
    assert g.sizes.grid_dim == G
    xyz = box_cloud(n, seed, G)
    rng = np.random.default_rng(seed)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    age[::17] = 0.5                                                       # some kids: exert and feel nothing
    ids = g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    order, f, lists, mom = frame(g)
    where = index_of(g, ids)
    assert len(order) == n and g.counters["cell_overflow_kills"] == 0
    g.close()
    kid = age < 1.5
    w_eff = np.where(kid, np.float32(0.0), np.float32(60.0)).astype(np.float32)
    return f, where[order], [where[l] for l in lists], xyz, w_eff, kid


def against_the_model(over, G, flags, seed, n=8192):
    f, idx, lists, xyz, w_eff, kid = model_frame(over, G, flags, seed, n)
    adults = np.nonzero(~kid[idx])[0]
    want = M.accel(lists, xyz, w_eff, G, 0.2, idx[adults])
    got = f[:, :3].astype(np.float64)
    rel = M.rel_dev(got[adults], want)
    cutoff = M.rel_dev(M.accel(lists, xyz, w_eff, G, 0.2, idx[adults], far=False), want)
    print("far monopoles, %d bodies on %d^3 cells, flags %#x: max relative deviation from the model %.3g (the stencil alone: median %.3g)"
          % (n, G, flags, rel.max(), np.median(cutoff)))
    assert (f[:, 3].view(np.int32) == 0).all() and not got[kid[idx]].any()
    return rel, f


GRIDS = [(SMALL, 8), (dict(max_particles_num=16384, chunk_factor=2, chunk_dim=3), 6), (dict(max_particles_num=16384, chunk_factor=1, chunk_dim=4), 4)]


@pytest.mark.parametrize("over,G", GRIDS, ids=["8^3", "6^3", "4^3"])
def test_force_records_follow_the_model(over, G):
    """8^3 cells: eight blocks of 64 cells in 16 parts, half of the parts empty; 6^3: no multiple of four, the last block
    ragged; 4^3: one block -- a corner cell's far set is 56 cells, an inner cell's 37.

    Every grid at the small contexts' density, about 16 bodies a cell: 8192, 3456 and 1024 bodies.  The bar is the
    project's for a particle's whole sum, and the stencil's part of that sum is the reference's serial fp32 chain, which
    this feature must leave bit for bit: the bar can be asked where the reference's own chain meets it.  At 16 a cell it
    does (432 additions).  At 8192 bodies on 4^3 cells (128 a cell, 3456 additions) it does not -- measured on an MI355X,
    the CUTOFF context's own record is 1.54e-5 of |a| away from the model's stencil sum for one particle of 7710, whose
    stencil sum is 4.3 times its whole |a|, and the far-monopole record 1.59e-5 (the next particle: 8.8e-6).  What this
    feature adds at that density has its own test below.  Measured: 8^3 4.3e-6."""
    rel, _ = against_the_model(over, G, FAR, 30 + G, 16 * G ** 3)
    assert rel.max() < REL


def test_the_far_part_alone_on_dense_cells():
    """8192 bodies on 4^3 cells, 128 a cell: what the far pass and the combine ADD to the stencil's chain -- the record of a
    far-monopole context minus the record of a cutoff context on the same cloud -- against the model's far part, on the
    scale of the particle's whole |a| (measured: 1.3e-6).  The stencil's chain drops out of the difference up to the
    rounding of the sixteen additions that carry it."""
    over, G = GRIDS[2]
    f, idx, lists, xyz, w_eff, kid = model_frame(over, G, FAR, 34, 8192)
    f0, idx0, _, _, _, _ = model_frame(over, G, 0, 34, 8192)
    assert np.array_equal(idx, idx0) and (f[:, 3].view(np.int32) == 0).all()
    adults = np.nonzero(~kid[idx])[0]
    whole = M.accel(lists, xyz, w_eff, G, 0.2, idx[adults])
    far = whole - M.accel(lists, xyz, w_eff, G, 0.2, idx[adults], far=False)
    got = f[adults, :3].astype(np.float64) - f0[adults, :3].astype(np.float64)
    rel = np.linalg.norm(got - far, axis=1) / np.linalg.norm(whole, axis=1)
    print("far part alone, 8192 bodies on 4^3 cells: max deviation from the model's far part over |a| %.3g" % rel.max())
    assert np.abs(far).max() > 0 and rel.max() < REL


# ---- 4. one adult per cell: the all-pairs force -----------------------------------------------------------------------------

def test_one_adult_per_cell_is_the_direct_sum():
    """no cell holds two: every monopole IS its cell's particle, the result is the all-pairs force up to association"""
    G = 16
    xyz = cloud(5000, 44, 39.98)
    _, first = np.unique(M.cells_of(xyz, G), return_index=True)
    xyz = xyz[np.sort(first)]
    n = len(xyz)
    assert 2500 < n < 3500
    g = ps.ParticleSystem(ps.default_config(flags=FAR, collision_radius=1e-6))
    ids = g.fill_particles(xyz, age=np.float32(3.0), fert_age=np.float32(1e6))
    order, f, lists, mom = frame(g)
    idx = index_of(g, ids)[order]
    occupied = np.nonzero(mom[:, 3] != 0)[0]
    assert len(occupied) == n and max(len(l) for l in lists) == 1
    assert np.array_equal(mom[M.cells_of(xyz, G)], np.concatenate([xyz, np.full((n, 1), 60.0, np.float32)], 1))
    want = M.direct(xyz, np.full(n, 60.0, np.float32), 0.2, idx)
    rel = M.rel_dev(f[:, :3].astype(np.float64), want)
    print("one adult per cell, %d bodies on 16^3 cells: max relative deviation from the fp64 direct sum %.3g" % (n, rel.max()))
    assert (f[:, 3].view(np.int32) == 0).all() and rel.max() < REL
    g.close()


# ---- 5. fast math -----------------------------------------------------------------------------------------------------------

def test_fast_math_follows_the_model_and_gives_the_same_bytes_twice():
    rel, f1 = against_the_model(SMALL, 8, FAR | ps.FLAG_FAST_MATH, 51)
    assert rel.max() < REL                                            # the tolerance mode's bar for uniform clouds (test_gpu_fast.py)
    _, f2 = against_the_model(SMALL, 8, FAR | ps.FLAG_FAST_MATH, 51)
    assert f1.tobytes() == f2.tobytes()


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------

def lively(n, seed, G):
    rng = np.random.default_rng(seed)
    age = rng.uniform(0.2, 9.0, n).astype(np.float32)
    return dict(xyz=box_cloud(n, seed, G), age=age, w=rng.uniform(20.0, 100.0, n).astype(np.float32),
                fert_age=rng.uniform(3.0, 12.0, n).astype(np.float32), vxyz=rng.uniform(-8, 8, (n, 3)).astype(np.float32))


def test_the_same_frame_gives_the_same_records_however_it_is_run():
    """plain stage calls; the slab family's calls with graphs on (captured, then replayed); run-ahead 0; after two steps
    and a snapshot_restore"""
    c = lively(8192, 61, 8)

    def records(graphs=False, run_ahead=1, detour=False):
        g = ps.ParticleSystem(ps.default_config(flags=FAR, **SMALL))
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
        return order.tobytes(), f.tobytes(), mom.tobytes()

    base = records()
    assert np.abs(np.frombuffer(base[1], np.float32)).max() > 0
    assert records(graphs=True) == base, "graphs on"
    assert records(run_ahead=0) == base, "run-ahead 0"
    assert records(detour=True) == base, "after snapshot_restore"


def test_three_steps_with_explosions_graphs_on_and_off():
    c = lively(8192, 62, 8)
    out = []
    for graphs in (False, True):
        g = ps.ParticleSystem(ps.default_config(flags=FAR | ps.FLAG_EXPLOSIONS, **SMALL))
        g.fill_particles(**c)
        if graphs:
            g.set_graphs(True)
        g.step(3)
        out.append((g.download_particles(), g.counters))
        if graphs:
            assert g.graph_stats()[0] > 0
        g.close()
    assert_same_particles(out[1][0], out[0][0], "three far-monopole steps with explosions, graphs on against off")
    assert out[0][1] == out[1][1] and out[0][1]["integrated"] > 5000


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------

def status_of_create(**over):
    with pytest.raises(ps.PsamdError) as e:
        ps.ParticleSystem(ps.default_config(**over))
    return e.value.status


def test_refusals():
    assert status_of_create(flags=FAR | ps.FLAG_ALL_PAIRS) == INVALID_ARG
    assert status_of_create(flags=FAR, world=2, rank=0) == UNSUPPORTED
    assert status_of_create(flags=FAR, eps2=1e-8) == UNSUPPORTED         # (eps2^3 below 2^-60: outside the lean range)
    g = ps.ParticleSystem(ps.default_config(flags=FAR, **SMALL))
    g.fill_particles(box_cloud(2000, 71, 8), age=np.float32(3.0), fert_age=np.float32(1e6))
    g.init_iframe(); g.build_grid()
    out = np.zeros((g.sizes.num_cells, 4), np.float32)
    assert g.lib.psamd_download_cell_moments(g.h, out.ctypes.data_as(ctypes.c_void_p)) == STATE      # before the pair stage
    assert g.lib.psamd_potential(g.h, ctypes.byref(ps.Potential())) == UNSUPPORTED
    assert g.lib.psamd_download_potential(g.h, None, 0, None) == UNSUPPORTED
    assert g.lib.psamd_probe(g.h, ctypes.byref(ps.ProbeSpec(fields=ps.PROBE_ACC, max_count=0))) == UNSUPPORTED
    g.calc_forces_pairs()
    assert (g.download_cell_moments()[:, 3] != 0).any()
    g.calc_forces_apply()
    assert g.lib.psamd_download_cell_moments(g.h, out.ctypes.data_as(ctypes.c_void_p)) == STATE      # the frame has ended
    g.step(1); g.synchronize()                                            # the context stayed usable
    assert g.counters["integrated"] >= 3900 and g.live_count() >= 1950
    g.close()
    b = ps.ParticleSystem(ps.default_config(**SMALL))
    b.fill_particles(box_cloud(2000, 71, 8), age=np.float32(3.0), fert_age=np.float32(1e6))
    b.init_iframe(); b.build_grid(); b.calc_forces_pairs()
    assert b.lib.psamd_download_cell_moments(b.h, out.ctypes.data_as(ctypes.c_void_p)) == UNSUPPORTED
    b.calc_forces_apply()
    b.close()


# ---- 8. one size up, once ---------------------------------------------------------------------------------------------------

def test_n_2_18_against_the_direct_sum_and_the_cutoff_steps_counters():
    """N = 2^18 on the default grid (64 to a cell): 200 served particles against an fp64 direct sum over all 2^18 bodies, the
    caps of the method (test_far_monopole_cpu.py); collisions are untouched, so the step's counters are the cutoff context's"""
    n = 1 << 18
    g = ps.ParticleSystem(ps.default_config(flags=FAR))
    b = ps.ParticleSystem(ps.default_config())
    xyz = g.uniform_cloud(n, 18)
    rng = np.random.default_rng(18)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    for s in (g, b):
        ids = s.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    order, f, _, _ = frame(g)
    b.step(1)
    cg, cb = g.counters, b.counters
    assert cg["integrated"] == cb["integrated"] > n // 2 and cg["deaths_collision"] == cb["deaths_collision"] > 0
    idx = index_of(g, ids)[order]
    served = np.nonzero(f[:, 3].view(np.int32) == 0)[0]
    pick = rng.choice(served, 200, replace=False)
    want = M.direct(xyz, np.full(n, 60.0, np.float32), 0.2, idx[pick], chunk=25)
    rel = M.rel_dev(f[pick, :3].astype(np.float64), want)
    print("far monopoles at N=2^18 vs fp64 direct sum (200 particles): median %.3g max %.3g" % (np.median(rel), rel.max()))
    assert rel.max() < 5e-2 and np.median(rel) < 5e-3
    g.close(); b.close()
