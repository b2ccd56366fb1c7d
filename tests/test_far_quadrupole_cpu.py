"""PSAMD_FLAG_FAR_QUADRUPOLE without a GPU: the header, the ctypes mirror and the library agree on the flag and on the new
entry point; the second moments of hand-made cells; and the METHOD -- the pyramid of monopoles plus the quadrupole term of
every far body (far_quadrupole_model.py) -- against an fp64 direct sum over all bodies.

The caps (median 2.2e-3, maximum 2.4e-2) are a property of the method, not of the device code: about 2x and 1.4x over the
worst measured, the margins test_far_pyramid_cpu.py uses; and on every cloud the median is at most half the pyramid's.
Measured with that file's clouds and seeds (8192 bodies, 400 sampled), median / maximum relative deviation of |a|, the
pyramid of monopoles -> with quadrupoles: 8^3 cells 2.39e-3 / 4.36e-2 -> 8.35e-4 / 1.38e-2 (uniform) and 1.97e-3 / 1.92e-2 ->
6.82e-4 / 5.08e-3 (clustered); 10^3 cells 5.12e-3 / 3.37e-2 -> 1.06e-3 / 1.17e-2 and 2.41e-3 / 2.62e-2 -> 7.56e-4 / 1.69e-2.  The
medians' ratios: 0.35, 0.35, 0.21, 0.31."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import far_monopole_model as M
import far_pyramid_model as Y
import far_quadrupole_model as Q
import particlesystem_amd as ps
from test_far_pyramid_cpu import clustered
from util import cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS2, W = 0.2, 60.0
NAME = "psamd_download_level_quadrupoles"


def test_header_mirror_and_library_agree_on_the_flag(tmp_path):
    ps.build()
    src = tmp_path / "flag.c"
    src.write_text('#include <stdio.h>\n#include "psamd.h"\nint main(void) {\n'
                   'int (*g)(psamd_ctx *, int32_t, void *) = psamd_download_level_quadrupoles; (void)g;\n'
                   'float out[6];\n'
                   'printf("%u %u %d %d\\n", PSAMD_FLAG_FAR_QUADRUPOLE, PSAMD_FLAG_FAR_QUADRUPOLE & (PSAMD_FLAG_EXPLOSIONS | '
                   'PSAMD_FLAG_FAST_MATH | PSAMD_FLAG_ALL_PAIRS | PSAMD_FLAG_EULER | PSAMD_FLAG_FAR_MONOPOLE | PSAMD_FLAG_FAR_PYRAMID), '
                   'psamd_abi_version(), psamd_download_level_quadrupoles(NULL, 0, out));\nreturn 0;\n}\n')
    exe = tmp_path / "flag"
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + os.path.dirname(ps.LIB_PATH), "-lpsamd", "-Wl,-rpath," + os.path.dirname(ps.LIB_PATH),
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)], check=True)
    flag, clash, abi, r = (int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert flag == ps.FLAG_FAR_QUADRUPOLE == 0x40 and clash == 0
    others = [getattr(ps, n) for n in dir(ps) if n.startswith("FLAG_") and n != "FLAG_FAR_QUADRUPOLE"]
    assert len(others) >= 6 and not any(ps.FLAG_FAR_QUADRUPOLE & o for o in others)
    assert abi == ps.ABI_VERSION == 8                                # one flag bit and one function: no layout moved
    assert r == 1                                                    # PSAMD_ERR_INVALID_ARG


def test_the_new_symbol_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "psamd.h")).read()
    ps.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", ps.LIB_PATH], check=True, capture_output=True, text=True).stdout
    lib = ps.load()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, text), NAME + " is not declared in the header"
    assert re.search(r" T %s$" % NAME, exported, re.M), NAME + " is not exported by the library"
    assert NAME in [n for n, _, _ in ps.ABI] and getattr(lib, NAME).restype is ctypes.c_int, NAME + " is not bound"
    assert lib.psamd_download_level_quadrupoles(None, 0, None) == 1  # PSAMD_ERR_INVALID_ARG
    out = (ctypes.c_float * 6)()
    assert lib.psamd_download_level_quadrupoles(None, 0, out) == 1
    assert callable(ps.ParticleSystem.download_level_quadrupoles)


def direct_central(xyz, w):
    """fp64 (X, Y, Z), M and the six central second moments of the bodies about their centre of mass, term by term"""
    x, w = np.asarray(xyz, np.float64), np.asarray(w, np.float64)
    com = (w[:, None] * x).sum(0) / w.sum()
    d = x - com
    return com, w.sum(), np.array([(w * d[:, a] * d[:, b]).sum() for a, b in Q.PLANES])


def test_hand_made_cells():
    """6^3 cells, levels 6 and 3 (test_far_pyramid_cpu.py's hand-made pyramid: every number a short dyadic, so that the
    float32 planes hold the moments exactly).  Two bodies in one cell: C = mu * delta_a * delta_b with the reduced mass
    mu = 20 * 60 / 80 and delta = (1, -1, 0.5); a single body: six exact zeros; a parent of two occupied cells: the moments of
    its three bodies about their centre of mass; repulsion flips all six planes and nothing else"""
    G = 6
    cell = lambda i1, i2, i3: (i3 * G + i1) * G + i2
    xyz = np.array([[-14.0, 14.0, 14.0], [-13.0, 13.0, 14.5], [-8.0, 9.0, 12.0], [1.0, 14.0, 14.0]], np.float32)
    w = np.array([20.0, 60.0, 80.0, 40.0], np.float32)
    lists = M.lists_of(xyz, G)
    assert [len(lists[c]) for c in (cell(0, 0, 0), cell(1, 1, 0), cell(0, 3, 0))] == [2, 1, 1]
    (m0, m1), (c0, c1) = Q.level_moments(lists, xyz, w, G)
    for a, b in zip((m0, m1), Y.level_moments(lists, xyz, w, G)):
        assert a.tobytes() == b.tobytes()                             # (X, Y, Z, M are the pyramid's)
    assert c0.dtype == c1.dtype == np.float32 and c0.shape == (216, 6) and c1.shape == (27, 6)
    assert c0[cell(0, 0, 0)].tolist() == [15.0, 15.0, 3.75, -15.0, 7.5, -7.5]
    for c in (cell(1, 1, 0), cell(0, 3, 0)):
        assert c0[c].tobytes() == bytes(24), "a single body has no second moments"
    assert np.count_nonzero(c0.any(1)) == 1
    com, mass, want = direct_central(xyz[:3], w[:3])
    assert m1[0].tolist() == com.tolist() + [mass]
    assert np.abs(c1[0].astype(np.float64) - want).max() <= 1e-9 * np.abs(want).max() and np.abs(want).min() > 1.0
    assert c1[1].tobytes() == bytes(24) and np.count_nonzero(c1.any(1)) == 1      # (the parent of the one body IS that body)
    (r0, r1), (q0, q1) = Q.level_moments(lists, xyz, -w, G)
    for a, b in ((r0, m0), (r1, m1)):
        assert np.array_equal(a[:, :3], b[:, :3]) and np.array_equal(a[:, 3], -b[:, 3])
    for a, b in ((q0, c0), (q1, c1)):
        assert np.array_equal(a, -b) and a.any()                      # (a zero stays +0: x - x is +0 under either sign)


def test_one_adult_per_cell_has_no_second_moments():
    """1000 random bodies, each alone: both products of C_ab round the same real number -- six exact zeros, whatever the bits"""
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-20, 20, (1000, 3)).astype(np.float32)
    w = rng.uniform(20, 100, 1000).astype(np.float32) * rng.choice([-1.0, 1.0], 1000).astype(np.float32)
    s = np.concatenate([Q.level_sums([np.array([k])], xyz, w, 1)[0] for k in range(1000)])
    assert (s[:, 0] != 0).all() and Q.central_of(s).tobytes() == bytes(24 * 1000)


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
    moments = Q.level_moments(lists, xyz, w, G)
    quad = M.rel_dev(Q.accel(lists, xyz, w, G, EPS2, pick, moments), want)
    mono = M.rel_dev(Y.accel(lists, xyz, w, G, EPS2, pick, levmom=moments[0]), want)
    print("%s cloud, %d bodies on %d^3 cells: with quadrupoles median %.3g max %.3g; the pyramid of monopoles median %.3g max %.3g"
          % (kind, n, G, np.median(quad), quad.max(), np.median(mono), mono.max()))
    assert np.median(quad) < 2.2e-3
    assert quad.max() < 2.4e-2
    assert np.median(quad) <= 0.5 * np.median(mono)
