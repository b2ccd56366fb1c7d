"""PSAMD_FLAG_FAR_MONOPOLE without a GPU: the header, the ctypes mirror and the library agree on the flag and on the new
entry point; and the METHOD -- the stencil as a direct sum, every other cell as one monopole (far_monopole_model.py) --
against an fp64 direct sum over all bodies.  The caps (median 5e-3, maximum 5e-2, the stencil alone above 0.5) are a
property of the method, not of the device code.  Measured with the seeds below, 400 particles sampled per cloud: median /
maximum relative deviation of |a| 2.1e-3 / 3.5e-2 on the uniform cloud and 1.5e-3 / 1.6e-2 on the clustered one; the
stencil alone: median 0.87 and 0.77."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import far_monopole_model as M
import particlesystem_amd as ps
from util import cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, EPS2, W = 8, 0.2, 60.0


def test_header_mirror_and_library_agree_on_the_flag(tmp_path):
    ps.build()
    src = tmp_path / "flag.c"
    src.write_text('#include <stdio.h>\n#include "psamd.h"\nint main(void) {\n'
                   'int (*f)(psamd_ctx *, void *) = psamd_download_cell_moments; (void)f;\n'
                   'printf("%u %u %d\\n", PSAMD_FLAG_FAR_MONOPOLE, PSAMD_FLAG_FAR_MONOPOLE & (PSAMD_FLAG_EXPLOSIONS | PSAMD_FLAG_FAST_MATH | '
                   'PSAMD_FLAG_ALL_PAIRS | PSAMD_FLAG_EULER), psamd_abi_version());\nreturn 0;\n}\n')
    exe = tmp_path / "flag"
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + os.path.dirname(ps.LIB_PATH), "-lpsamd", "-Wl,-rpath," + os.path.dirname(ps.LIB_PATH),
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)], check=True)
    flag, clash, abi = (int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert flag == ps.FLAG_FAR_MONOPOLE == 0x10 and clash == 0
    assert abi == ps.ABI_VERSION == 8                                # one flag bit and one function: no layout moved


def test_the_new_symbol_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "psamd.h")).read()
    ps.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", ps.LIB_PATH], check=True, capture_output=True, text=True).stdout
    lib = ps.load()
    name = "psamd_download_cell_moments"
    assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in the header"
    assert re.search(r" T %s$" % name, exported, re.M), name + " is not exported by the library"
    assert name in [n for n, _, _ in ps.ABI] and getattr(lib, name).restype is ctypes.c_int, name + " is not bound"
    assert lib.psamd_download_cell_moments(None, None) == 1          # PSAMD_ERR_INVALID_ARG
    assert callable(ps.ParticleSystem.download_cell_moments)


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


@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_the_method_against_the_direct_sum(kind):
    n, half = 8192, G * 2.5 * 0.9995
    xyz = cloud(n, 11, half) if kind == "uniform" else clustered(n, 12, half)
    w = np.full(n, W, np.float32)
    lists = M.lists_of(xyz, G)
    assert sum(len(l) for l in lists) == n
    pick = np.random.default_rng(13).choice(n, 400, replace=False)
    want = M.direct(xyz, w, EPS2, pick)
    far = M.rel_dev(M.accel(lists, xyz, w, G, EPS2, pick), want)
    near = M.rel_dev(M.accel(lists, xyz, w, G, EPS2, pick, far=False), want)
    print("%s cloud, %d bodies on %d^3 cells: stencil + far monopoles median %.3g max %.3g; stencil alone median %.3g"
          % (kind, n, G, np.median(far), far.max(), np.median(near)))
    assert np.median(far) < 5e-3
    assert far.max() < 5e-2
    assert np.median(near) > 0.5


def test_the_moments_of_a_hand_made_frame():
    """one adult: its own position and mass, exactly; kids only: zeros; the centre of mass of two; repulsion flips M alone"""
    xyz = np.array([[1.25, -2.5, 3.0], [7.0, 7.0, 7.0], [6.0, 8.0, 9.0], [-12.0, 1.0, 1.0], [-13.0, 2.0, 1.5]], np.float32)
    w = np.array([60.0, 0.0, 0.0, 20.0, 60.0], np.float32)
    lists = [np.array([0]), np.array([1, 2]), np.array([3, 4]), np.array([], np.int64)]
    m = M.moments(lists, xyz, w)
    assert m[0].tolist() == [1.25, -2.5, 3.0, 60.0]
    assert not m[1].any() and not m[3].any()
    assert m[2].tolist() == [np.float32((20.0 * -12.0 + 60.0 * -13.0) / 80.0), 1.75, np.float32((20.0 + 90.0) / 80.0), 80.0]
    r = M.moments(lists, xyz, -w)
    assert np.array_equal(r[:, :3], m[:, :3]) and np.array_equal(r[:, 3], -m[:, 3])
