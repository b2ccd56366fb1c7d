"""The far-field force on the device, what the suites of the three methods share (test_gpu_far_monopole.py,
test_gpu_far_pyramid.py, test_gpu_far_quadrupole.py; include/psamd.h: "long-range gravity", "a pyramid of monopoles", "quadrupoles on
the pyramid"): the moment planes of every level bit for bit against the numpy model (far_model.py), no far cell (the cutoff
context's bytes), the force records against the model's fp64 sums (1e-5 relative, the project's bar for sums of this kind), the
far part alone, lanes of one wave under different parents, fast math, determinism and the refusals; and, for
test_gpu_far_rough.py, the same against the model on rough frames (section 7: deep grids, collisions, clumps, repulsion).

METHODS has one row per method.  Every check below is written once and takes the method; tests_of(method) makes the row's
cases of them into test functions, which the method's suite takes into its namespace beside the tests only that method has.
The three suites stay three files so that every test keeps the node id it has had.  The contexts, grids and clouds are
far_harness.py's (8^3 cells of about 16 bodies unless noted)."""
import ctypes
import functools

import numpy as np
import pytest

import far_model as F
import oracle_py as O
import particlesystem_amd as ps
from far_harness import (DEEP, GRID, INVALID_ARG, STATE, UNSUPPORTED, box_cloud, crowd_and_nursery, frame, index_of, lively, model_frame,
                         rough_bodies, rough_frame, status_of_create, waves_of)
from util import assert_same_particles, oracle_cfg_from

MONO, PYR, QUADRUPOLE = ps.FLAG_FAR_MONOPOLE, ps.FLAG_FAR_PYRAMID, ps.FLAG_FAR_QUADRUPOLE
QUAD = PYR | QUADRUPOLE
REL = 1e-5

# method (far_model.py's name): its row.
#   flags       of a context of the method
#   name        in messages
#   moments     {G: bodies} of the moments check
#   records     {G: bodies} of force_records_follow_the_model: about 16 a cell (16^3: 4)
#   dense       (G, bodies) of the_far_part_alone_on_dense_cells, or None
#   parents     whether a cell has a parent (lanes_of_one_wave_under_different_parents)
#   planes_of   the flags of the context whose X, Y, Z, M the method's are, byte for byte, or None
#   download    the method's own download of a level's planes as the C ABI has it, and the width of a row
#   filled      what the planes of a frame of 2000 bodies on 8^3 cells must show
#   without     the flags of contexts that refuse that download
#   create      creations the method refuses beside the common ones: (config, status)
#   services    whether the far potential and the far probe are refused too (they are served on flat and pyramid contexts)
METHODS = {
    "flat": dict(
        flags=MONO, name="far monopoles", moments={8: 6000}, records={8: 8192, 6: 3456, 4: 1024}, dense=(4, 8192), parents=False,
        planes_of=None, download=lambda g, level, vp: g.lib.psamd_download_cell_moments(g.h, vp), width=4,
        filled=lambda g: (g.download_cell_moments()[:, 3] != 0).any(), without=(0,), create=[], services=False),
    "pyramid": dict(
        flags=PYR, name="pyramid", moments={8: 6144, 10: 12000}, records={6: 3456, 8: 8192, 10: 16000, 16: 16384}, dense=(8, 16384),
        parents=True, planes_of=None,
        download=lambda g, level, vp: g.lib.psamd_download_level_moments(g.h, level, vp), width=4,
        filled=lambda g: (g.download_level_moments(1)[:, 3] != 0).all(), without=(0, MONO),
        create=[(dict(flags=PYR | MONO), INVALID_ARG),
                (dict(flags=PYR, collision_radius=4.0), UNSUPPORTED)],      # (no two-pass pair stage)
        services=False),
    "quadrupole": dict(
        flags=QUAD, name="quadrupoles", moments={8: 6144, 10: 12000}, records={6: 3456, 8: 8192, 10: 16000, 16: 16384}, dense=None,
        parents=True, planes_of=PYR,
        download=lambda g, level, vp: g.lib.psamd_download_level_quadrupoles(g.h, level, vp), width=6,
        filled=lambda g: g.download_level_quadrupoles(1)[:, :3].all(), without=(0, PYR),
        create=[(dict(flags=QUADRUPOLE), INVALID_ARG),                      # the flag alone
                (dict(flags=QUADRUPOLE | MONO), INVALID_ARG),
                (dict(flags=QUAD | MONO), INVALID_ARG),
                (dict(flags=QUAD, collision_radius=4.0), UNSUPPORTED)],
        services=True),
}


# ---- 1. moments -------------------------------------------------------------------------------------------------------

def planes_are_the_models(got, want, dims, width, what):
    """every level's planes, every word"""
    for l, (have, exp) in enumerate(zip(got, want)):
        assert have.shape == exp.shape == (dims[l] ** 3, width)
        bad = np.nonzero((have.view(np.uint32) != exp.view(np.uint32)).any(1))[0]
        assert len(bad) == 0, ("level %d: %s differ from the model in %d cells, first %d: device %r model %r"
                               % (l, what, len(bad), bad[0], have[bad[0]], exp[bad[0]]))


def moments_of_every_level_equal_the_model_bit_for_bit(method, G, n, sign):
    """kids among the adults, unequal masses, one cell of kids only (its planes are all zeros); on 8^3 one cell with more
    particles than its list holds (only the first MAX_PARTICLES_PER_CELL count; the list is longer than 64, so the sums take a
    second round of lanes).  10^3: level 1 has 5 cells an axis, so level 2's last parents have one child an axis.  Level 0 is
    the flat method's and psamd_download_cell_moments'; a quadrupole context's X, Y, Z and M are a plain pyramid context's bytes"""
    row = METHODS[method]
    dims = F.levels(G, method)
    cap = ps.describe(ps.default_config(**GRID[G]))[0].max_per_cell
    xyz, age, w, full, kids_only = crowd_and_nursery(n, G, cap)
    got = {}
    for flags in [row["flags"]] + [f for f in [row["planes_of"]] if f is not None]:
        g = ps.ParticleSystem(ps.default_config(flags=flags, force_sign=sign, collision_radius=1e-6, **GRID[G]))
        assert g.sizes.grid_dim == G and g.sizes.max_per_cell == cap
        ids = g.fill_particles(xyz, age=age, w=w, fert_age=np.float32(1e6))
        fr = frame(g, apply=False)
        cells = g.download_cell_moments()
        g.calc_forces_apply()
        if G == 8:
            assert cap > 64 and len(fr.lists[full]) == cap and g.counters["cell_overflow_kills"] >= 14
        got[flags] = (index_of(g, ids), fr, cells)
        g.close()
    where, fr, cells = got[row["flags"]]
    if row["planes_of"] is not None:
        other = got[row["planes_of"]][1]
        assert other.cen is None and b"".join(m.tobytes() for m in fr.mom) == b"".join(m.tobytes() for m in other.mom)
    lists = [where[l] for l in fr.lists]
    w_eff = np.where(age < 1.5, np.float32(0.0), np.float32(sign) * w).astype(np.float32)
    want_mom, want_cen = F.level_moments(lists, xyz, w_eff, G, method)
    assert np.array_equal(want_mom[0], F.level_moments(lists, xyz, w_eff, G, "flat")[0][0]) and cells.tobytes() == fr.mom[0].tobytes()
    assert not want_mom[0][kids_only].any() and want_mom[0][full, 3] != 0 and (want_mom[0][:, 3] != 0).sum() > 400
    assert len(fr.mom) == len(want_mom) == len(dims) and (fr.cen is None) == (want_cen is None)
    planes_are_the_models(fr.mom, want_mom, dims, 4, "moments")
    for exp in want_mom:
        assert (exp[:, 3] != 0).all() or exp is want_mom[0]
        assert ((exp[:, 3] > 0) == (sign > 0))[exp[:, 3] != 0].all()
    if want_cen is not None:
        assert not want_cen[0][kids_only].any() and want_cen[0][full].all()
        planes_are_the_models(fr.cen, want_cen, dims, 6, "second moments")
        for exp in want_cen:
            diag = exp[:, :3]
            assert (np.sign(diag[diag != 0]) == sign).all() and (diag != 0).any()      # (Caa has M's sign)


# ---- 2. no far cell: the cutoff result -----------------------------------------------------------------------------------

def confined_cloud_is_the_cutoff_result_byte_for_byte(method):
    """a cloud inside a 2x2x2 block of cells of the default 16^3 grid (cells 7..8 on every axis: two parents at every level):
    every cell of the block is in every other's stencil, and no ancestor of a stencil cell is in the set -- the force records and
    the whole step are the cutoff context's, whatever the planes hold; flat: and the oracle's"""
    n = 3000
    rng = np.random.default_rng(7)
    xyz = rng.uniform(-4.99, 4.99, (n, 3)).astype(np.float32)           # cells 7..8 on every axis
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    a = ps.ParticleSystem(ps.default_config(flags=METHODS[method]["flags"]))
    b = ps.ParticleSystem(ps.default_config())
    for s in (a, b):
        s.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    fa, fb = frame(a), frame(b)
    assert np.array_equal(fa.order, fb.order) and np.abs(fa.f[:, :3]).max() > 0 and fa.f.tobytes() == fb.f.tobytes()
    assert [int((m[:, 3] != 0).sum()) for m in fa.mom] == [8] * len(F.levels(16, method))
    if fa.cen is not None:
        assert [int(c[:, :3].all(1).sum()) for c in fa.cen] == [8, 8, 8]
    assert_same_particles(a.download_particles(), b.download_particles(), "%s step on a confined cloud" % METHODS[method]["name"])
    if method == "flat":
        o = O.System(oracle_cfg_from(b.cfg))
        o.fill(xyz, age=age, fert_age=np.float32(1e6))
        o.step(1)
        assert_same_particles(a.download_particles(), o.particles, "far-monopole step on a confined cloud")
        o.close()
    a.close(); b.close()


# ---- 3. against the model ---------------------------------------------------------------------------------------------------

def against_the_model(method, G, flags, seed, n):
    f, idx, lists, xyz, w_eff, kid = model_frame(G, flags, seed, n)
    adults = np.nonzero(~kid[idx])[0]
    moments = F.level_moments(lists, xyz, w_eff, G, method)
    want = F.accel(lists, xyz, w_eff, G, 0.2, idx[adults], method, moments)
    got = f[:, :3].astype(np.float64)
    rel = F.rel_dev(got[adults], want)
    if method == "quadrupole":
        share = np.linalg.norm(F.quad_accel(lists, xyz, w_eff, G, 0.2, idx[adults], moments), axis=1) / np.linalg.norm(want, axis=1)
        beside = "the quadrupole part: median %.3g of |a|" % np.median(share)
    else:
        cutoff = F.rel_dev(F.accel(lists, xyz, w_eff, G, 0.2, idx[adults], method, far=False), want)
        beside = "the stencil alone: median %.3g" % np.median(cutoff)
    print("%s, %d bodies on %d^3 cells, flags %#x: max relative deviation from the model %.3g (%s)"
          % (METHODS[method]["name"], n, G, flags, rel.max(), beside))
    assert (f[:, 3].view(np.int32) == 0).all() and not got[kid[idx]].any()
    if method == "quadrupole":
        assert np.median(share) > 1e-4                                   # (the part is there to be got wrong)
    if method == "pyramid":
        assert np.median(cutoff) > 0.1                                   # (the far part is no small correction here)
    return rel, f


def force_records_follow_the_model(method, G, n):
    """Every grid at the small contexts' density, about 16 bodies a cell (16^3: 4, 16384 bodies).  4^3: one block -- a corner
    cell's flat far set is 56 cells, an inner cell's 37; 6^3: levels 6, 3, and flat no multiple of four, the last block ragged;
    8^3: levels 8, 4, and flat eight blocks of 64 cells in 16 parts, half of the parts empty; 10^3: 10, 5, 3 with ragged parents;
    16^3: three levels, 64 blocks at level 0, of which a wave walks a few.

    The bar is the project's for a particle's whole sum, and the stencil's part of that sum is the reference's serial fp32
    chain, which this feature must leave bit for bit: the bar can be asked where the reference's own chain meets it.  At 16 a
    cell it does (432 additions).  At 8192 bodies on 4^3 cells (128 a cell, 3456 additions) it does not -- measured on an MI355X,
    the CUTOFF context's own record is 1.54e-5 of |a| away from the model's stencil sum for one particle of 7710, whose stencil
    sum is 4.3 times its whole |a|, and the far-monopole record 1.59e-5 (the next particle: 8.8e-6).  What the far field adds at
    that density has its own test below.

    Measured on an MI355X: flat 8^3 4.3e-6; pyramid 6^3 2.3e-6, 8^3 4.3e-6, 10^3 2.1e-6, 16^3 1.1e-6; quadrupole 6^3 2.2e-6, 8^3
    4.2e-6, 10^3 2.0e-6, 16^3 1.2e-6 (the quadrupole part: 0.2-0.5 % of |a| for the median particle)"""
    rel, _ = against_the_model(method, G, METHODS[method]["flags"], 30 + G, n)
    assert rel.max() < REL


def the_far_part_alone_on_dense_cells(method, G, n):
    """flat: 8192 bodies on 4^3 cells, 128 a cell; pyramid: 16384 bodies on 8^3 cells, 32 a cell.  What the far pass (the walk)
    and the combine ADD to the stencil's chain -- the record of a far context minus the record of a cutoff context on the same
    cloud -- against the model's far part, on the scale of the particle's whole |a|, so that a wrong mask cannot hide behind a
    large stencil sum (measured: flat 1.3e-6, pyramid 1.8e-6).  The stencil's chain drops out of the difference up to the
    rounding of the sixteen additions that carry it."""
    f, idx, lists, xyz, w_eff, kid = model_frame(G, METHODS[method]["flags"], 34, n)
    f0, idx0, _, _, _, _ = model_frame(G, 0, 34, n)
    assert np.array_equal(idx, idx0) and (f[:, 3].view(np.int32) == 0).all()
    adults = np.nonzero(~kid[idx])[0]
    whole = F.accel(lists, xyz, w_eff, G, 0.2, idx[adults], method)
    far = whole - F.accel(lists, xyz, w_eff, G, 0.2, idx[adults], method, far=False)
    got = f[adults, :3].astype(np.float64) - f0[adults, :3].astype(np.float64)
    rel = np.linalg.norm(got - far, axis=1) / np.linalg.norm(whole, axis=1)
    print("%s, far part alone, %d bodies on %d^3 cells: max deviation from the model's far part over |a| %.3g"
          % (METHODS[method]["name"], n, G, rel.max()))
    assert np.abs(far).max() > 0 and rel.max() < REL


def lanes_of_one_wave_under_different_parents(method):
    """700 bodies on 8^3 cells, one or two a cell: the 64 served particles of a wave come from some 50 cells, which lie under
    several parents at either level -- every lane masks by its own parent, and its members -- of both chains -- are its own
    (measured on an MI355X: pyramid 7.2e-7, quadrupole 7.1e-7)"""
    G, n = 8, 700
    f, idx, lists, xyz, w_eff, kid = model_frame(G, METHODS[method]["flags"], 35, n)
    cells = F.cells_of(xyz[idx], G)
    assert (np.diff(cells) >= 0).all()                                   # (sorted order: the dense tasks take the served ones in it)
    i1, i2, i3 = (cells // G % G) >> 1, (cells % G) >> 1, (cells // (G * G)) >> 1
    assert len(np.unique(((i3 * 4 + i1) * 4 + i2)[:64])) >= 8            # one wave's worth of particles, many parents
    adults = np.nonzero(~kid[idx])[0]
    want = F.accel(lists, xyz, w_eff, G, 0.2, idx[adults], method)
    rel = F.rel_dev(f[adults, :3].astype(np.float64), want)
    print("%s, sparse cloud, %d bodies on %d^3 cells: max relative deviation from the model %.3g" % (METHODS[method]["name"], n, G, rel.max()))
    assert (f[:, 3].view(np.int32) == 0).all() and rel.max() < REL


# ---- 4. fast math -----------------------------------------------------------------------------------------------------------

def fast_math_follows_the_model_and_gives_the_same_bytes_twice(method):
    """Measured on an MI355X: quadrupole 3.1e-6"""
    flags = METHODS[method]["flags"] | ps.FLAG_FAST_MATH
    rel, f1 = against_the_model(method, 8, flags, 51, 8192)
    assert rel.max() < REL                                            # the tolerance mode's bar for uniform clouds (test_gpu_fast.py)
    _, f2 = against_the_model(method, 8, flags, 51, 8192)
    assert f1.tobytes() == f2.tobytes()


# ---- 5. determinism ---------------------------------------------------------------------------------------------------------

def the_same_frame_gives_the_same_records_however_it_is_run(method):
    """plain stage calls; the slab family's calls with graphs on (captured, then replayed); run-ahead 0; after two steps
    and a snapshot_restore -- the records and all planes of every level"""
    c = lively(8192, 61, 8)

    def records(graphs=False, run_ahead=1, detour=False):
        g = ps.ParticleSystem(ps.default_config(flags=METHODS[method]["flags"], **GRID[8]))
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
        fr = frame(g, slab=graphs)
        if graphs:
            assert g.graph_stats()[0] > 0
        g.close()
        return fr.order.tobytes(), fr.f.tobytes(), b"".join(m.tobytes() for m in fr.mom), b"".join(m.tobytes() for m in fr.cen or [])

    base = records()
    assert np.abs(np.frombuffer(base[1], np.float32)).max() > 0
    assert (len(base[3]) > 0) == (method == "quadrupole") and (not base[3] or np.frombuffer(base[3], np.float32).any())
    assert records(graphs=True) == base, "graphs on"
    assert records(run_ahead=0) == base, "run-ahead 0"
    assert records(detour=True) == base, "after snapshot_restore"


def three_steps_with_explosions_graphs_on_and_off(method):
    c = lively(8192, 62, 8)
    out = []
    for graphs in (False, True):
        g = ps.ParticleSystem(ps.default_config(flags=METHODS[method]["flags"] | ps.FLAG_EXPLOSIONS, **GRID[8]))
        g.fill_particles(**c)
        if graphs:
            g.set_graphs(True)
        g.step(3)
        out.append((g.download_particles(), g.counters))
        if graphs:
            assert g.graph_stats()[0] > 0
        g.close()
    assert_same_particles(out[1][0], out[0][0], "three %s steps with explosions, graphs on against off" % METHODS[method]["name"])
    assert out[0][1] == out[1][1] and out[0][1]["integrated"] > 5000


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------

def refusals(method):
    row = METHODS[method]
    far, download = row["flags"], row["download"]
    assert status_of_create(flags=far | ps.FLAG_ALL_PAIRS) == INVALID_ARG
    assert status_of_create(flags=far, world=2, rank=0) == UNSUPPORTED
    assert status_of_create(flags=far, eps2=1e-8) == UNSUPPORTED         # (eps2^3 below 2^-60: outside the lean range)
    for config, status in row["create"]:
        assert status_of_create(**config) == status, config
    g = ps.ParticleSystem(ps.default_config(flags=far, **GRID[8]))
    g.fill_particles(box_cloud(2000, 71, 8), age=np.float32(3.0), fert_age=np.float32(1e6))
    g.init_iframe(); g.build_grid()
    out = np.zeros((g.sizes.num_cells, row["width"]), np.float32)
    vp = out.ctypes.data_as(ctypes.c_void_p)
    assert download(g, 0, vp) == STATE                                    # before the pair stage
    assert g.lib.psamd_download_cell_moments(g.h, vp) == STATE
    assert g.lib.psamd_potential(g.h, ctypes.byref(ps.Potential())) == UNSUPPORTED
    assert g.lib.psamd_download_potential(g.h, None, 0, None) == UNSUPPORTED
    assert g.lib.psamd_probe(g.h, ctypes.byref(ps.ProbeSpec(fields=ps.PROBE_ACC, max_count=0))) == UNSUPPORTED
    if row["services"]:
        assert g.lib.psamd_potential(g.h, ctypes.byref(ps.Potential(flags=ps.POTENTIAL_FAR))) == UNSUPPORTED
        assert g.lib.psamd_download_potential_far(g.h, None, 0, None) == UNSUPPORTED
        assert g.lib.psamd_probe(g.h, ctypes.byref(ps.ProbeSpec(fields=ps.PROBE_ACC | ps.PROBE_FAR, max_count=0))) == UNSUPPORTED
    g.calc_forces_pairs()
    if row["parents"]:
        assert download(g, -1, vp) == INVALID_ARG
        assert download(g, 2, vp) == INVALID_ARG                          # (levels 8, 4: L = 1)
        assert download(g, 0, None) == INVALID_ARG
    assert row["filled"](g)
    g.calc_forces_apply()
    assert download(g, 0, vp) == STATE                                    # the frame has ended
    g.step(1); g.synchronize()                                            # the context stayed usable
    assert g.counters["integrated"] >= 3900 and g.live_count() >= 1950
    g.close()
    for flags in row["without"]:
        b = ps.ParticleSystem(ps.default_config(flags=flags, **GRID[8]))
        b.fill_particles(box_cloud(2000, 71, 8), age=np.float32(3.0), fert_age=np.float32(1e6))
        b.init_iframe(); b.build_grid(); b.calc_forces_pairs()
        assert download(b, 0, vp) == UNSUPPORTED
        b.calc_forces_apply()
        b.close()


# ---- 7. the rough frames (test_gpu_far_rough.py) ------------------------------------------------------------------------------------
# Deep grids, collisions at the default radius, clumps, repulsion: the frames are far_harness.rough_frame's, one per (cloud, grid,
# flags), and the model's moments of each are formed once.  Every bar is REL.

@functools.lru_cache(maxsize=None)
def rough_moments(kind, G, method, sign=1.0):
    s = rough_frame(kind, G, METHODS[method]["flags"], sign)
    return F.level_moments(s.lists, s.xyz, s.w_eff, G, method)


def rough_planes_are_the_models(method, s, moments, G):
    dims = F.levels(G, method)
    want_mom, want_cen = moments
    assert len(s.mom) == len(want_mom) == len(dims) and (s.cen is None) == (want_cen is None)
    planes_are_the_models(s.mom, want_mom, dims, 4, "moments")
    if want_cen is not None:
        assert len(s.cen) == len(dims)
        planes_are_the_models(s.cen, want_cen, dims, 6, "second moments")
    return dims, [int((m[:, 3] != 0).sum()) for m in want_mom]


def deep_moments_equal_the_model_bit_for_bit(method, G):
    """Four and five levels (far_harness.DEEP): far_level's padded offsets behind level 2, k_level_moments over three and four upper
    levels, on 36^3 two odd levels below the top -- 9 and 5 -- whose last parents have one child an axis.  A level's planes read at
    another level's offset, or a ragged parent that took a child of the next row, differ in whole cells"""
    n, levels, cap = DEEP[G]
    cfg = ps.default_config(**GRID[G])
    assert ps.far_levels(cfg) == levels == F.levels_of(G) and ps.describe(cfg)[0].max_per_cell == cap
    s = rough_frame("deep", G, METHODS[method]["flags"])
    dims, filled = rough_planes_are_the_models(method, s, rough_moments("deep", G, method), G)
    print("%s, %d bodies on %d^3 cells: levels %r, cells with mass %r, every word the model's" % (METHODS[method]["name"], n, G, dims, filled))
    assert len(s.idx) == n and s.kid.sum() > 400 and all(filled) and (method == "flat" or filled[-1] == dims[-1] ** 3)


def deep_sample(s, G):
    """the served adults (positions in the sorted order) whose records are compared: every particle of the first and of the last
    wave, of every wave that crosses an i3-layer boundary -- its box falls back to the full range on the other axes --, and 1024
    more by a seeded choice; beside them the number of crossing waves"""
    served = np.nonzero(~s.kid[s.idx])[0]
    _, span = waves_of(F.cells_of(s.xyz[s.idx[served]], G), G)
    wave = np.arange(len(served)) // 64
    crossing = np.nonzero(span > 1)[0]
    pick = (wave == 0) | (wave == wave[-1]) | np.isin(wave, crossing)
    pick[np.random.default_rng(93).choice(len(served), 1024, replace=False)] = True
    return served[pick], len(crossing)


def sampled_records_against_the_model(method, s, G, kind, at):
    """(the relative deviation of the records `at` -- positions in the sorted order -- from the model, of the stencil alone)"""
    want = F.accel(s.lists, s.xyz, s.w_eff, G, 0.2, s.idx[at], method, rough_moments(kind, G, method))
    near = F.accel(s.lists, s.xyz, s.w_eff, G, 0.2, s.idx[at], method, far=False)
    return F.rel_dev(s.f[at, :3].astype(np.float64), want), F.rel_dev(near, want)


def deep_force_records_follow_the_model(method, G, fast=0):
    """The walk on four and five levels: far_box below the top with l = 1 and 2 (the shift by l + 1), far_blocks of levels that are
    neither the top nor level 0, and the wave box's fall-back -- at one body a cell or fewer a wave's 64 served particles span a
    whole layer, and the waves that cross to the next layer take the full range on the other two axes.  Flat on 20^3: 125 blocks,
    so the sixteen parts are ragged, floor(125 p / 16).  The far part is nearly all of |a| here (the stencil alone is off by more
    than 0.9 for the median particle), so a level left out or taken twice cannot hide.
    Measured on an MI355X: see CHANGELOG.md"""
    flags = METHODS[method]["flags"] | fast
    s = rough_frame("deep", G, flags)
    at, crossing = deep_sample(s, G)
    rel, alone = sampled_records_against_the_model(method, s, G, "deep", at)
    print("%s, %d bodies on %d^3 cells, flags %#x: %d records sampled, %d waves cross a layer; max relative deviation from the model "
          "%.3g (the stencil alone: median %.3g)" % (METHODS[method]["name"], len(s.idx), G, flags, len(at), crossing, rel.max(), np.median(alone)))
    assert (s.f[:, 3].view(np.int32) == 0).all() and not s.f[s.kid[s.idx], :3].any() and crossing >= G // 2
    assert np.median(alone) > 0.9
    assert rel.max() < REL
    if fast:
        again = rough_frame.__wrapped__("deep", G, flags)
        assert again.f.tobytes() == s.f.tobytes()


def collisions_at_the_default_radius(method):
    """8192 bodies on 8^3 cells at collision_radius 0.4 (far_harness.COLLIDE_SEED), a far context and a cutoff context on the same
    fill.  The served subset -- dense_gi, the r index of part_acc -- now skips collided adults as well as kids, and a collided adult
    still exerts (w_eff looks at the age alone).  (a) the flag words are the cutoff context's, and the oracle's; (b) every record
    that is not served, a kid's or a flagged one, is the cutoff context's 16 bytes; (c) every served record follows the model
    with the collided adults' mass in; (d) the planes are the model's with that mass in, bit for bit; (e) the test can tell: at
    least 200 adults collided, and the model without their mass is more than 10 * REL away from the device for more than half of
    the served particles"""
    G = 8
    s, s0 = rough_frame("collide", G, METHODS[method]["flags"]), rough_frame("collide", G, 0)
    assert np.array_equal(s.idx, s0.idx)
    flag, kid = s.f[:, 3].view(np.int32), s.kid[s.idx]
    assert flag.tobytes() == s0.f[:, 3].view(np.int32).tobytes() == oracle_flags_of_the_colliding_cloud(G).tobytes()      # (a)
    served, collided = ~kid & (flag == 0), ~kid & (flag != 0)
    assert s.f[~served].tobytes() == s0.f[~served].tobytes() and (flag[kid] == 0).all()      # (b)
    assert collided.sum() >= 200 and kid.sum() > 400                      # (e)
    rough_planes_are_the_models(method, s, rough_moments("collide", G, method), G)      # (d)
    at = np.nonzero(served)[0]
    want = F.accel(s.lists, s.xyz, s.w_eff, G, 0.2, s.idx[at], method, rough_moments("collide", G, method))
    rel = F.rel_dev(s.f[at, :3].astype(np.float64), want)                 # (c)
    less = s.w_eff.copy()
    less[s.idx[collided]] = 0.0
    without = F.accel(s.lists, s.xyz, less, G, 0.2, s.idx[at], method)
    away = F.rel_dev(s.f[at, :3].astype(np.float64), without)
    print("%s, %d bodies on %d^3 cells at the default collision radius: %d adults collided, %d served; max relative deviation from the "
          "model %.3g; from the model without the collided adults' mass: median %.3g, %.3f of the served beyond 10 * REL"
          % (METHODS[method]["name"], len(s.idx), G, collided.sum(), len(at), rel.max(), np.median(away), (away > 10 * REL).mean()))
    assert rel.max() < REL
    assert (away > 10 * REL).mean() > 0.5                                 # (e)


@functools.lru_cache(maxsize=None)
def oracle_flags_of_the_colliding_cloud(G):
    """the flag words of the sorted order from the CPU oracle (the reference's own scan)"""
    c, over = rough_bodies("collide", G)
    o = O.System(oracle_cfg_from(ps.default_config(**{**GRID[G], **over})))
    o.fill(c["xyz"], age=c["age"], fert_age=c["fert_age"], w=c["w"])
    o.init_iframe(); o.build_grid()
    f = np.zeros((o.sorted_count(), 4), np.float32)
    o.calc_pairs(0, len(f), f)
    o.close()
    return f[:, 3].view(np.int32).copy()


def clumps_follow_the_model_whole_and_in_the_far_part(method, kind):
    """8^3 cells, six Gaussian clusters (far_harness.clustered(4096, 12): the fullest cell holds 44, the corners none) and
    rough_cloud(), the same clusters with one cell filled to 65 adults and 36 adults alone in three layers.  Check 1: every whole
    record against the model at REL -- the stencil's serial fp32 chain, the reference's own, is at most 5.3e-6 of |a| from the model's
    fp64 stencil sum on the clusters and 2.9e-6 on the rough cloud (measured with the CPU oracle), the far part adds 1-2e-6.  Check
    2: the far part alone, the record minus the cutoff context's record on the same fill, over the whole |a|: a wrong mask cannot
    hide behind a large stencil sum.  rough_cloud(): some wave's box is a single cell (no lane falls back), and some wave spans
    three or more i3 layers (every lane falls back on two axes): asserted from the sorted cells.  On the plain clusters no wave can
    do either -- at most 44 bodies a cell, more than 64 served a layer"""
    G = 8
    s, s0 = rough_frame(kind, G, METHODS[method]["flags"]), rough_frame(kind, G, 0)
    assert np.array_equal(s.idx, s0.idx) and (s.f[:, 3].view(np.int32) == 0).all()
    at = np.nonzero(~s.kid[s.idx])[0]
    cells, span = waves_of(F.cells_of(s.xyz[s.idx[at]], G), G)
    if kind == "rough":
        assert cells[0] == 1 and span.max() >= 3
    whole = F.accel(s.lists, s.xyz, s.w_eff, G, 0.2, s.idx[at], method, rough_moments(kind, G, method))
    far = whole - F.accel(s.lists, s.xyz, s.w_eff, G, 0.2, s.idx[at], method, far=False)
    rel = F.rel_dev(s.f[at, :3].astype(np.float64), whole)
    got = s.f[at, :3].astype(np.float64) - s0.f[at, :3].astype(np.float64)
    part = np.linalg.norm(got - far, axis=1) / np.linalg.norm(whole, axis=1)
    print("%s, %s cloud, %d bodies on %d^3 cells: a wave's cells %d..%d, layers up to %d; max relative deviation from the model %.3g; "
          "the far part alone, over |a|: %.3g" % (METHODS[method]["name"], kind, len(s.idx), G, cells.min(), cells.max(), span.max(), rel.max(), part.max()))
    assert np.abs(far).max() > 0 and rel.max() < REL
    assert part.max() < REL


def repulsion_in_the_force_records(method, G):
    """force_sign = -1 on 8^3 and 10^3 cells, about 16 bodies a cell: the records against the model with w_eff = -w -- the sign rides
    on the moments' M and, for quadrupoles, on C -- and every served record points away from the model's attractive record"""
    s = rough_frame("repel", G, METHODS[method]["flags"], -1.0)
    at = np.nonzero(~s.kid[s.idx])[0]
    assert (s.w_eff[~s.kid] < 0).all() and (s.f[:, 3].view(np.int32) == 0).all()
    want = F.accel(s.lists, s.xyz, s.w_eff, G, 0.2, s.idx[at], method, rough_moments("repel", G, method, -1.0))
    pull = F.accel(s.lists, s.xyz, -s.w_eff, G, 0.2, s.idx[at], method)
    got = s.f[at, :3].astype(np.float64)
    rel = F.rel_dev(got, want)
    cos = (got * pull).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(pull, axis=1))
    print("%s, repulsion, %d bodies on %d^3 cells: max relative deviation from the model %.3g; cosine to the attractive record at most %.6f"
          % (METHODS[method]["name"], len(s.idx), G, rel.max(), cos.max()))
    assert rel.max() < REL
    assert ((got * pull).sum(1) < 0).all()


# ---- the cases of a row as tests ------------------------------------------------------------------------------------------------

def tests_of(method):
    """{name: test function}: the row's cases of the checks above, for the namespace of the method's suite"""
    row = METHODS[method]

    def case(check, *args):
        def test():
            check(method, *args)
        test.__doc__ = check.__doc__
        return "test_" + check.__name__, test

    @pytest.mark.parametrize("sign", [1.0, -1.0])
    @pytest.mark.parametrize("G", list(row["moments"]))
    def moments(G, sign):
        moments_of_every_level_equal_the_model_bit_for_bit(method, G, row["moments"][G], sign)

    @pytest.mark.parametrize("G", list(row["records"]), ids=lambda G: "%d^3" % G)
    def records(G):
        force_records_follow_the_model(method, G, row["records"][G])

    moments.__doc__ = moments_of_every_level_equal_the_model_bit_for_bit.__doc__
    records.__doc__ = force_records_follow_the_model.__doc__
    tests = dict([case(confined_cloud_is_the_cutoff_result_byte_for_byte), case(fast_math_follows_the_model_and_gives_the_same_bytes_twice),
                  case(the_same_frame_gives_the_same_records_however_it_is_run), case(three_steps_with_explosions_graphs_on_and_off),
                  case(refusals)],
                 test_moments_of_every_level_equal_the_model_bit_for_bit=moments, test_force_records_follow_the_model=records)
    if row["dense"]:
        tests.update([case(the_far_part_alone_on_dense_cells, *row["dense"])])
    if row["parents"]:
        tests.update([case(lanes_of_one_wave_under_different_parents)])
    return tests
