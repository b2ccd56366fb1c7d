"""PSAMD_FLAG_FAR_PYRAMID without a GPU: the header, the ctypes mirror and the library agree on the flag and on the two new
entry points; psamd_far_levels; the partition property of the interaction set; and the METHOD -- the stencil as a direct
sum, coarser monopoles for farther mass (far_pyramid_model.py) -- against an fp64 direct sum over all bodies.

The caps (median 1e-2, maximum 6e-2, the stencil alone above 0.5) are a property of the method, not of the device code: about
2x and 1.4x over the worst measured, the margins test_far_monopole_cpu.py uses.  Measured with the seeds below, 8192 bodies, 400
sampled per cloud, median / maximum relative deviation of |a|: 8^3 cells 2.4e-3 / 4.4e-2 (uniform) and 2.0e-3 / 1.9e-2
(clustered); 10^3 cells (levels 10, 5, 3: an odd level with a ragged parent) 5.1e-3 / 3.4e-2 and 2.4e-3 / 2.6e-2; the stencil
alone: median 0.77 to 0.92."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import far_monopole_model as M
import far_pyramid_model as Y
import particlesystem_amd as ps
from util import cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS2, W = 0.2, 60.0
NAMES = ("psamd_far_levels", "psamd_download_level_moments")


def test_header_mirror_and_library_agree_on_the_flag(tmp_path):
    ps.build()
    src = tmp_path / "flag.c"
    src.write_text('#include <stdio.h>\n#include "psamd.h"\nint main(void) {\n'
                   'int (*f)(const psamd_config *, int32_t *, int32_t *) = psamd_far_levels; (void)f;\n'
                   'int (*g)(psamd_ctx *, int32_t, void *) = psamd_download_level_moments; (void)g;\n'
                   'int32_t n = 0, dims[16];\n'
                   'printf("%u %u %d %d %d\\n", PSAMD_FLAG_FAR_PYRAMID, PSAMD_FLAG_FAR_PYRAMID & (PSAMD_FLAG_EXPLOSIONS | PSAMD_FLAG_FAST_MATH | '
                   'PSAMD_FLAG_ALL_PAIRS | PSAMD_FLAG_EULER | PSAMD_FLAG_FAR_MONOPOLE), psamd_abi_version(), '
                   'psamd_far_levels(NULL, &n, dims), psamd_download_level_moments(NULL, 0, dims));\nreturn 0;\n}\n')
    exe = tmp_path / "flag"
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + os.path.dirname(ps.LIB_PATH), "-lpsamd", "-Wl,-rpath," + os.path.dirname(ps.LIB_PATH),
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)], check=True)
    flag, clash, abi, r1, r2 = (int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert flag == ps.FLAG_FAR_PYRAMID == 0x20 and clash == 0
    assert abi == ps.ABI_VERSION == 8                                # one flag bit and two functions: no layout moved
    assert r1 == 1 and r2 == 1                                       # PSAMD_ERR_INVALID_ARG


def test_the_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "psamd.h")).read()
    ps.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", ps.LIB_PATH], check=True, capture_output=True, text=True).stdout
    lib = ps.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in the header"
        assert re.search(r" T %s$" % name, exported, re.M), name + " is not exported by the library"
        assert name in [n for n, _, _ in ps.ABI] and getattr(lib, name).restype is ctypes.c_int, name + " is not bound"
    assert lib.psamd_far_levels(None, None, None) == 1               # PSAMD_ERR_INVALID_ARG
    assert lib.psamd_download_level_moments(None, 0, None) == 1
    assert callable(ps.ParticleSystem.download_level_moments) and callable(ps.far_levels)


@pytest.mark.parametrize("factor,dim,want", [(1, 4, [4]), (2, 3, [6, 3]), (2, 4, [8, 4]), (2, 5, [10, 5, 3]), (4, 4, [16, 8, 4]),
                                             (8, 5, [40, 20, 10, 5, 3])])
def test_far_levels(factor, dim, want):
    cfg = ps.default_config(chunk_factor=factor, chunk_dim=dim)
    assert ps.describe(cfg)[0].grid_dim == want[0]
    assert ps.far_levels(cfg) == want == Y.levels_of(want[0])
    n, dims = ctypes.c_int32(), (ctypes.c_int32 * 16)(*([-1] * 16))
    assert ps.load().psamd_far_levels(ctypes.byref(cfg), ctypes.byref(n), dims) == 0
    assert n.value == len(want) and list(dims) == want + [0] * (16 - len(want))


@pytest.mark.parametrize("G", [4, 6, 8, 10, 16])
def test_stencil_and_set_cover_every_cell_exactly_once(G):
    sizes = []
    for c in range(G ** 3):
        members = Y.interaction_set(c, G)
        n = Y.coverage(c, G, members)
        assert (n == 1).all(), "cell %d of %d^3: %d cells not covered once" % (c, G, (n != 1).sum())
        sizes.append(len(members))
    print("%d^3 cells: %.0f far bodies a particle in the mean (flat: %.0f)"
          % (G, np.mean(sizes), np.mean([G ** 3 - len(M.stencil_cells(c, G)) for c in range(G ** 3)])))


def clustered(n, seed, half):
    """test_far_monopole_cpu.py's: six Gaussian clusters (sigma = 7.5) with centres in the inner half of the box; draws
    outside the box are dropped"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-half / 2, half / 2, (6, 3))
    xyz = centres[rng.integers(0, 6, 3 * n)] + rng.normal(0.0, 7.5, (3 * n, 3))
    xyz = xyz[(np.abs(xyz) < half).all(1)][:n]
    assert len(xyz) == n
    return xyz.astype(np.float32)


@pytest.mark.parametrize("G", [8, 10])
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_the_method_against_the_direct_sum(kind, G):
    n, half = 8192, G * 2.5 * 0.9995
    xyz = cloud(n, 11, half) if kind == "uniform" else clustered(n, 12, half)
    w = np.full(n, W, np.float32)
    lists = M.lists_of(xyz, G)
    assert sum(len(l) for l in lists) == n
    pick = np.random.default_rng(13).choice(n, 400, replace=False)
    want = M.direct(xyz, w, EPS2, pick)
    far = M.rel_dev(Y.accel(lists, xyz, w, G, EPS2, pick), want)
    near = M.rel_dev(Y.accel(lists, xyz, w, G, EPS2, pick, far=False), want)
    print("%s cloud, %d bodies on %d^3 cells: stencil + pyramid median %.3g max %.3g; stencil alone median %.3g"
          % (kind, n, G, np.median(far), far.max(), np.median(near)))
    assert np.median(far) < 1e-2
    assert far.max() < 6e-2
    assert np.median(near) > 0.5


def test_a_hand_made_pyramid():
    """6^3 cells, levels 6 and 3.  Two occupied cells under one parent: the parent is their joint centre of mass, the sums
    taken in child order; one occupied cell under another parent: the parent IS that cell; the cells' own moments are
    far_monopole_model's; repulsion flips M alone, at every level"""
    G = 6
    cell = lambda i1, i2, i3: (i3 * G + i1) * G + i2
    xyz = np.array([[-14.0, 14.0, 14.0], [-13.0, 13.0, 14.5], [-8.0, 9.0, 12.0], [1.0, 14.0, 14.0]], np.float32)
    w = np.array([20.0, 60.0, 80.0, 40.0], np.float32)
    assert M.cells_of(xyz, G).tolist() == [cell(0, 0, 0), cell(0, 0, 0), cell(1, 1, 0), cell(0, 3, 0)]
    lists = M.lists_of(xyz, G)
    m0, m1 = Y.level_moments(lists, xyz, w, G)
    assert np.array_equal(m0, M.moments(lists, xyz, w))
    assert m0[cell(0, 0, 0)].tolist() == [-13.25, 13.25, 14.375, 80.0]
    assert m1[0].tolist() == [np.float32((20.0 * -14.0 + 60.0 * -13.0 + 80.0 * -8.0) / 160.0), 11.125, 13.1875, 160.0]
    assert m1[1].tolist() == [1.0, 14.0, 14.0, 40.0] == m0[cell(0, 3, 0)].tolist()
    assert (m1[:, 3] != 0).sum() == 2 and (m0[:, 3] != 0).sum() == 3
    r0, r1 = Y.level_moments(lists, xyz, -w, G)
    for a, b in ((r0, m0), (r1, m1)):
        assert np.array_equal(a[:, :3], b[:, :3]) and np.array_equal(a[:, 3], -b[:, 3])
