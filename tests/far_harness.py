"""What the far-field suites share (far_force_suite.py, far_field_suite.py, test_gpu_far_*.py, test_far_*_cpu.py): the small
contexts, one frame of any far context, the clouds, what the field services' tests read their results with, the two checks of a
feature's C surface and the checks of the method without a
GPU.  The numpy model is far_model.py."""
import collections
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import far_model as F
import particlesystem_amd as ps
from service_harness import DEV, bits, open_frame  # noqa: F401  (for the suites)
from service_harness import ERR_INVALID_ARG as INVALID_ARG, ERR_STATE as STATE, ERR_UNSUPPORTED as UNSUPPORTED  # noqa: F401
from util import cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the small contexts hold max_particles_num=16384; the grids are 4^3 (one level), 6^3 (levels 6, 3), 8^3 (8, 4), 10^3 (10, 5, 3: an odd
# level with a ragged parent) and 16^3 (16, 8, 4); the deep grids (DEEP) are 20^3, 24^3, 32^3 and 36^3
GRID = {4: dict(max_particles_num=16384, chunk_factor=1, chunk_dim=4),
        6: dict(max_particles_num=16384, chunk_factor=2, chunk_dim=3),
        8: dict(max_particles_num=16384, chunk_factor=2, chunk_dim=4),
        10: dict(max_particles_num=16384, chunk_factor=2, chunk_dim=5),
        16: dict(max_particles_num=16384, chunk_factor=4, chunk_dim=4, x_factor=8),      # (x_factor: lists of 40, for 4 a cell in the mean)
        20: dict(max_particles_num=16384, chunk_factor=5, chunk_dim=4, x_factor=8),
        24: dict(max_particles_num=16384, chunk_factor=6, chunk_dim=4, x_factor=8),
        32: dict(max_particles_num=16384, chunk_factor=8, chunk_dim=4, x_factor=8),
        36: dict(max_particles_num=16384, chunk_factor=9, chunk_dim=4, x_factor=8)}
# the deep grids, four and five levels: G -> (bodies of its uniform cloud, the levels, the lists' cap).  20^3: an odd level (5) with a
# ragged parent, and flat 125 blocks over 16 parts; 24^3: the grid of the benchmark's cloud at N = 2^22; 36^3: two odd levels below the
# top (9 and 5).  About one body a cell or fewer: a wave's 64 served particles span a layer of cells or more
DEEP = {20: (8000, [20, 10, 5, 3], 24), 24: (13824, [24, 12, 6, 3], 16), 32: (16384, [32, 16, 8, 4], 8), 36: (16000, [36, 18, 9, 5, 3], 8)}
Frame = collections.namedtuple("Frame", "order f lists mom cen")


def make(G, flags, **over):
    g = ps.ParticleSystem(ps.default_config(flags=flags, collision_radius=1e-6, **GRID[G], **over))
    assert g.sizes.grid_dim == G
    return g


def frame(g, apply=True, slab=False):
    """one frame up to the pair stage: (slot ids in sorted order, force records, cell lists as slot ids, the levels' (X, Y, Z, M) --
    one level on a flat context -- or None on a context without far monopoles, the levels' six C planes on a quadrupole context
    or None)"""
    if slab:
        g.slab_build(); g.slab_pairs()
    else:
        open_frame(g); g.calc_forces_pairs()
    rows = g.download_cellgrid()
    lists = [row[1:1 + row[0]] for row in rows]
    order = np.concatenate(lists)
    f = g.download_force4(0, len(order))
    levels = range(len(ps.far_levels(g.cfg)))
    mom = cen = None
    if g.cfg.flags & ps.FLAG_FAR_PYRAMID:
        mom = [g.download_level_moments(l) for l in levels]
    elif g.cfg.flags & ps.FLAG_FAR_MONOPOLE:
        mom = [g.download_cell_moments()]
    if g.cfg.flags & ps.FLAG_FAR_QUADRUPOLE:
        cen = [g.download_level_quadrupoles(l) for l in levels]
    if apply:
        if slab:
            g.slab_apply(); g.slab_finish()
        else:
            g.calc_forces_apply()
    return Frame(order, f, lists, mom, cen)


def index_of(g, ids):
    """slot id -> index into the arrays the fill was given"""
    where = np.full(g.sizes.container_size, -1, np.int64)
    where[ids] = np.arange(len(ids))
    return where


def fill_lists(g, ids):
    """(the lists as indices into the fill, the sorted order as indices into the fill)"""
    where = index_of(g, ids)
    lists = [where[row[1:1 + row[0]]] for row in g.download_cellgrid()]
    return lists, np.concatenate(lists)


def box_cloud(n, seed, G):
    return cloud(n, seed, G * 2.5 * 0.9995)


def low_corner(i1, i2, i3, G):
    """of a cell (i2 ~ +x, i1 ~ -y, i3 ~ -z)"""
    return np.array([(i2 - G // 2) * 5.0, -(i1 - G // 2) * 5.0 - 5.0, -(i3 - G // 2) * 5.0 - 5.0])


def lively(n, seed, G):
    rng = np.random.default_rng(seed)
    age = rng.uniform(0.2, 9.0, n).astype(np.float32)
    return dict(xyz=box_cloud(n, seed, G), age=age, w=rng.uniform(20.0, 100.0, n).astype(np.float32),
                fert_age=rng.uniform(3.0, 12.0, n).astype(np.float32), vxyz=rng.uniform(-8, 8, (n, 3)).astype(np.float32))


def clustered(n, seed, half):
    """Six Gaussian clusters with centres in the inner half of the box; draws outside the box are dropped.  sigma = 7.5, a
    cell and a half: a cluster is then wider than a stencil (15 units), which is the case the far field is for -- a cluster
    that fits one stencil has most of its pull inside the cutoff already."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-half / 2, half / 2, (6, 3))
    xyz = centres[rng.integers(0, 6, 3 * n)] + rng.normal(0.0, 7.5, (3 * n, 3))
    xyz = xyz[(np.abs(xyz) < half).all(1)][:n]
    assert len(xyz) == n
    return xyz.astype(np.float32)


def crowd_and_nursery(n, G, cap):
    """the cloud of the moments tests (seed 21): n uniform bodies, kids among the adults, unequal masses; the cell `full` emptied
    and given a crowd -- on 8^3 of cap + 14, more than its list holds and more than 64, else of 20 --, the cell `kids_only` emptied
    and given five kids.  (xyz, age, w, full, kids_only)"""
    rng = np.random.default_rng(21)
    xyz = box_cloud(n, 21, G)
    cell = F.cells_of(xyz, G)
    full, kids_only = (3 * G + 4) * G + 2, (5 * G + 1) * G + 6
    xyz = xyz[(cell != full) & (cell != kids_only)]
    n_crowd = cap + 14 if G == 8 else 20
    crowd = (low_corner(4, 2, 3, G) + rng.uniform(0.05, 4.95, (n_crowd, 3))).astype(np.float32)
    nursery = (low_corner(1, 6, 5, G) + rng.uniform(0.05, 4.95, (5, 3))).astype(np.float32)
    age = rng.uniform(15 / 7, 7.5, len(xyz)).astype(np.float32)
    age[::13] = 0.5
    xyz = np.concatenate([xyz, crowd, nursery])
    age = np.concatenate([age, np.full(len(crowd), 3.0, np.float32), np.full(5, 0.5, np.float32)])
    assert (F.cells_of(crowd, G) == full).all() and (F.cells_of(nursery, G) == kids_only).all()
    w = rng.uniform(20.0, 100.0, len(xyz)).astype(np.float32)
    return xyz, age, w, full, kids_only


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
    fr = frame(g)
    where = index_of(g, ids)
    assert len(fr.order) == n and g.counters["cell_overflow_kills"] == 0
    g.close()
    kid = age < 1.5
    w_eff = np.where(kid, np.float32(0.0), np.float32(60.0)).astype(np.float32)
    return fr.f, where[fr.order], [where[l] for l in fr.lists], xyz, w_eff, kid


def body_cloud(n, seed, G):
    """kids among the adults (they exert nothing and get the field at their own place), unequal masses"""
    rng = np.random.default_rng(seed)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    age[::17] = 0.5
    return dict(xyz=box_cloud(n, seed, G), age=age, w=rng.uniform(20.0, 100.0, n).astype(np.float32), fert_age=np.float32(1e6))


# ---- the rough frames (test_gpu_far_rough.py): deep grids, collisions, clumps, repulsion ------------------------------------------------

RoughFrame = collections.namedtuple("RoughFrame", "f idx lists mom cen xyz w w_eff kid")


def rough_cloud():
    """8^3 cells: clustered(4096, 12) without its bodies in cell 0 and in the layers i3 >= 5, then 65 adults in cell 0 -- the first
    cell of the sorted order, one short of its list's cap: the first wave's 64 served particles are in ONE cell -- and 36 adults
    spread over the layers i3 = 5, 6, 7: fewer than 64 behind layer 4, so the last wave spans three layers or more.
    (xyz, age)"""
    G = 8
    rng = np.random.default_rng(91)
    xyz = clustered(4096, 12, G * 2.5 * 0.9995)
    cell = F.cells_of(xyz, G)
    xyz = xyz[(cell != 0) & (cell // (G * G) < 5)]
    age = rng.uniform(15 / 7, 7.5, len(xyz)).astype(np.float32)
    age[::17] = 0.5
    crowd = (low_corner(0, 0, 0, G) + rng.uniform(0.05, 4.95, (65, 3))).astype(np.float32)
    haze = rng.uniform(-19.9, 19.9, (36, 3))
    haze[:, 2] = rng.uniform(-19.9, -5.1, 36)                             # (i3 ~ -z: layers 5..7)
    xyz = np.concatenate([crowd, xyz, haze.astype(np.float32)])
    age = np.concatenate([np.full(65, 3.0, np.float32), age, np.full(36, 3.0, np.float32)])
    layer = F.cells_of(xyz, G) // (G * G)
    assert (F.cells_of(crowd, G) == 0).all() and (layer[-36:] >= 5).all() and (layer >= 5).sum() == 36
    return xyz, age


@functools.lru_cache(maxsize=None)
def rough_bodies(kind, G):
    """(the fill of a rough frame, what its configuration has beside GRID[G]).  Every cloud has unequal masses and kids
    (age[::17] = 0.5) among the adults.
    deep     DEEP's uniform cloud on a deep grid
    collide  lively's cloud of 8192 on 8^3 cells at the DEFAULT collision radius, 0.4
    clump    clustered(4096, 12) on 8^3 cells
    rough    rough_cloud() on 8^3 cells
    repel    a uniform cloud, about 16 bodies a cell (for force_sign = -1)"""
    over = dict(collision_radius=1e-6)
    if kind == "collide":
        c, over = lively(8192, COLLIDE_SEED, G), {}
        c["age"] = np.random.default_rng(COLLIDE_SEED).uniform(15 / 7, 7.5, 8192).astype(np.float32)      # (adults: the more to collide)
        c["age"][::17] = 0.5
        return c, over
    rng = np.random.default_rng(92 + G)
    if kind == "deep":
        return body_cloud(DEEP[G][0], 90 + G, G), over
    if kind == "repel":
        return body_cloud(16 * G ** 3, 95 + G, G), over
    xyz, age = rough_cloud() if kind == "rough" else (clustered(4096, 12, G * 2.5 * 0.9995), None)
    if age is None:
        age = rng.uniform(15 / 7, 7.5, len(xyz)).astype(np.float32)
        age[::17] = 0.5
    return dict(xyz=xyz, age=age, w=rng.uniform(20.0, 100.0, len(xyz)).astype(np.float32), fert_age=np.float32(1e6)), over


COLLIDE_SEED = 65          # (chosen with the oracle on the CPU: 260 of the 7710 adults collide)


@functools.lru_cache(maxsize=None)
def rough_frame(kind, G, flags, sign=1.0):
    """one frame of rough_bodies(kind, G) on a context of `flags`: the records in sorted order, their index into the fill, the lists
    as indices into the fill, the planes of every level; positions, masses, w_eff (force_sign folded in, kids 0; a collided adult
    keeps its mass) and the kid mask in the order of the fill.  Computed once, never changed."""
    c, over = rough_bodies(kind, G)
    g = ps.ParticleSystem(ps.default_config(flags=flags, force_sign=sign, **{**GRID[G], **over}))
    assert g.sizes.grid_dim == G
    ids = g.fill_particles(**c)
    fr = frame(g)
    where = index_of(g, ids)
    assert len(fr.order) == len(ids) and g.counters["cell_overflow_kills"] == 0
    g.close()
    kid = c["age"] < 1.5
    w_eff = np.where(kid, np.float32(0.0), np.float32(sign) * c["w"]).astype(np.float32)
    return RoughFrame(fr.f, where[fr.order], [where[l] for l in fr.lists], fr.mom, fr.cen, c["xyz"], c["w"], w_eff, kid)


def waves_of(cells, G):
    """the dense tasks of the force walk -- the served particles' cells in sorted order, 64 to a wave --: per wave (the number of
    cells, the i3 layers from its lowest to its highest cell)"""
    assert (np.diff(cells) >= 0).all()
    first = np.arange(0, len(cells), 64)
    layer = cells // (G * G)
    return (np.array([len(np.unique(cells[k:k + 64])) for k in first]),
            np.maximum.reduceat(layer, first) - np.minimum.reduceat(layer, first) + 1)


# ---- the field services' results (psamd_potential, psamd_probe) ----------------------------------------------------------------------

def by_fill(ids, phi):
    """phi pairs with the live particles in ascending slot id: back to the order of the fill"""
    out = np.empty(len(ids), np.float32)
    out[np.argsort(ids)] = np.asarray(phi.cpu().numpy() if isinstance(phi, torch.Tensor) else phi)
    return out


def pos4_of(xyz):
    p = np.zeros((len(xyz), 4), np.float32)
    p[:, :3] = xyz
    return torch.from_numpy(p).to(DEV)


def record(res):
    return {k: res[k] for k in res if k != "phi"}


def served(g, far):
    """the potential and the probe keywords of a context's own far form"""
    return dict(far=far, quadrupole=bool(g.cfg.flags & ps.FLAG_FAR_QUADRUPOLE))


def status_of_create(**over):
    with pytest.raises(ps.PsamdError) as e:
        ps.ParticleSystem(ps.default_config(**over))
    return e.value.status


# ---- a feature's C surface, without a GPU ---------------------------------------------------------------------------------------

def c_prints(tmp_path, body):
    """the integers a C program prints whose main() is `body`, compiled against include/psamd.h and linked with the library"""
    ps.build()
    src = tmp_path / "snippet.c"
    src.write_text('#include <stdio.h>\n#include "psamd.h"\nint main(void) {\n' + body + 'return 0;\n}\n')
    exe = tmp_path / "snippet"
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + os.path.dirname(ps.LIB_PATH), "-lpsamd", "-Wl,-rpath," + os.path.dirname(ps.LIB_PATH),
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)], check=True)
    return [int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]


def declared_exported_bound(names):
    """every name is declared in the header, exported by the library and bound in ps.ABI; returns the loaded library"""
    text = open(os.path.join(ROOT, "include", "psamd.h")).read()
    ps.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", ps.LIB_PATH], check=True, capture_output=True, text=True).stdout
    lib = ps.load()
    for name in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in the header"
        assert re.search(r" T %s$" % name, exported, re.M), name + " is not exported by the library"
        assert name in [n for n, _, _ in ps.ABI] and getattr(lib, name).restype is ctypes.c_int, name + " is not bound"
    return lib


# ---- the method without a GPU (the test_far_*_cpu.py suites) -----------------------------------------------------------------------

EPS2, W = 0.2, 60.0


def cloud_frame(kind, G, n=8192):
    half = G * 2.5 * 0.9995
    xyz = cloud(n, 11, half) if kind == "uniform" else clustered(n, 12, half)
    lists = F.lists_of(xyz, G)
    assert sum(len(l) for l in lists) == n
    return xyz, np.full(n, W, np.float32), lists


def method_against_the_direct_sum(method, kind, G):
    """8192 bodies of equal mass, 400 of them sampled: the relative deviations of |a| from the fp64 direct sum over all bodies of
    (the method, beside it the stencil alone -- quadrupole: the pyramid's monopoles alone)"""
    xyz, w, lists = cloud_frame(kind, G)
    pick = np.random.default_rng(13).choice(len(xyz), 400, replace=False)
    want = F.direct(xyz, w, EPS2, pick)
    moments = F.level_moments(lists, xyz, w, G, method)
    far = F.rel_dev(F.accel(lists, xyz, w, G, EPS2, pick, method, moments), want)
    if method == "quadrupole":
        beside = F.rel_dev(F.accel(lists, xyz, w, G, EPS2, pick, "pyramid", (moments[0], None)), want)
    else:
        beside = F.rel_dev(F.accel(lists, xyz, w, G, EPS2, pick, method, far=False), want)
    print("%s cloud, %d bodies on %d^3 cells, %s: median %.3g max %.3g; %s median %.3g max %.3g"
          % (kind, len(xyz), G, method, np.median(far), far.max(), "the pyramid of monopoles" if method == "quadrupole" else "the stencil alone",
             np.median(beside), beside.max()))
    return far, beside


@functools.lru_cache(maxsize=None)
def phi_against_the_direct_sum(kind, G):
    """8192 bodies of equal mass, 400 of them sampled: {a method, or "stencil": the relative deviations of its fp64 phi from the fp64
    direct sum over all bodies}.  Computed once, never changed."""
    xyz, w, lists = cloud_frame(kind, G)
    pick = np.random.default_rng(13).choice(len(xyz), 400, replace=False)
    cell = F.cells_of(xyz, G)[pick]
    want = F.direct_phi(xyz, w, EPS2, pick)
    dev = {method: F.phi64(lists, xyz, w, G, EPS2, xyz[pick], cell, pick, method) for method in F.METHODS}
    dev["stencil"] = F.phi64(lists, xyz, w, G, EPS2, xyz[pick], cell, pick, "flat", far=False)
    return {k: np.abs(got - want) / np.abs(want) for k, got in dev.items()}


def two_forms_of_the_model_agree(method):
    """the fp32 association against the fp64 form, both signs of w; kids among the points (w_eff 0: they see every body).  The
    bound is one for every method (far_model.ALLOW): a quadrupole term is a small part of phi, and its own rounding -- some ten
    operations of 2^-24 each on a term of at most a few 1e-3 of phi -- is far below what the monopole chains are allowed"""
    G = 8
    xyz, w, lists = cloud_frame("uniform", G, 4096)
    w = w.copy()
    w[::17] = 0.0
    pick = np.concatenate([np.arange(0, 170, 17), np.random.default_rng(14).choice(len(xyz), 190, replace=False)])
    cell = F.cells_of(xyz, G)[pick]
    for sign in (1.0, -1.0):
        a = F.phi64(lists, xyz, np.float32(sign) * w, G, EPS2, xyz[pick], cell, pick, method)
        b = F.phi32(lists, xyz, np.float32(sign) * w, G, EPS2, xyz[pick], cell, pick, method)
        rel = np.abs(b - a) / np.abs(a)
        beside = ""
        if method == "quadrupole":
            part = F.quad_sum64(lists, xyz, np.float32(sign) * w, G, EPS2, xyz[pick], cell)
            beside = " (the quadrupole part: median %.3g of |phi|)" % np.median(np.abs(part / a))
            assert np.abs(part).min() > 0
        print("%s, sign %+.0f: fp32 association against fp64, max %.3g%s" % (method, sign, rel.max(), beside))
        assert b.dtype == np.float32 and (np.sign(a) == -sign).all() and rel.max() < F.ALLOW


def hand_made_pyramid():
    """6^3 cells, levels 6 and 3, every number a short dyadic: (G, cell(i1, i2, i3), xyz, w).  Two bodies in cell (0, 0, 0) and one in
    (1, 1, 0) under one parent, one in (0, 3, 0) under another"""
    G = 6
    xyz = np.array([[-14.0, 14.0, 14.0], [-13.0, 13.0, 14.5], [-8.0, 9.0, 12.0], [1.0, 14.0, 14.0]], np.float32)
    w = np.array([20.0, 60.0, 80.0, 40.0], np.float32)
    return G, lambda i1, i2, i3: (i3 * G + i1) * G + i2, xyz, w
