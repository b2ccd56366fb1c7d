"""PSAMD_POTENTIAL_FAR / PSAMD_PROBE_FAR without a GPU: the header, the ctypes mirror and the library agree on the two new
bits and on psamd_download_potential_far (ABI 8: no layout moved); the model's two forms agree; and the METHOD -- the
stencil as a direct sum, the far set's monopoles behind it (far_potential_model.py) -- against an fp64 direct sum over all
bodies: the far phi is nearer to it than the stencil-only phi, for the median particle, flat and as a pyramid.

Measured with the seeds below, 8192 bodies, 400 sampled per cloud, median / maximum relative deviation of phi from the
direct sum -- flat; pyramid; the stencil alone:
  8^3 uniform     1.1e-4 / 5.7e-4;  1.8e-4 / 1.1e-3;  0.87 / 0.94
  8^3 clustered   1.1e-4 / 7.2e-4;  2.7e-4 / 1.1e-3;  0.78 / 0.98
  10^3 uniform    8.6e-5 / 4.2e-4;  1.1e-3 / 5.2e-3;  0.91 / 0.96
  10^3 clustered  1.0e-4 / 5.1e-4;  4.4e-4 / 2.9e-3;  0.82 / 0.99
The model's fp32 association against its fp64 form: 1.3e-7 (flat), 1.9e-7 (pyramid)"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import far_monopole_model as M
import far_potential_model as F
import particlesystem_amd as ps
from test_far_pyramid_cpu import clustered
from util import cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS2, W = 0.2, 60.0


def test_header_mirror_and_library_agree_on_the_bits(tmp_path):
    ps.build()
    src = tmp_path / "bits.c"
    src.write_text('#include <stdio.h>\n#include "psamd.h"\nint main(void) {\n'
                   'int (*f)(psamd_ctx *, float *, int64_t, psamd_potential_result *) = psamd_download_potential_far; (void)f;\n'
                   'printf("%u %u %u %d %d %zu %zu\\n", PSAMD_POTENTIAL_FAR, PSAMD_PROBE_FAR, PSAMD_PROBE_FAR & (PSAMD_PROBE_ACC | PSAMD_PROBE_PHI), '
                   'psamd_abi_version(), psamd_download_potential_far(NULL, NULL, 0, NULL), sizeof(psamd_potential_spec), sizeof(psamd_probe_spec));\n'
                   'return 0;\n}\n')
    exe = tmp_path / "bits"
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + os.path.dirname(ps.LIB_PATH), "-lpsamd", "-Wl,-rpath," + os.path.dirname(ps.LIB_PATH),
                    "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)], check=True)
    pot, prb, clash, abi, rc, s1, s2 = (int(t) for t in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert pot == ps.POTENTIAL_FAR == 0x1 and prb == ps.PROBE_FAR == 0x4 and clash == 0
    assert abi == ps.ABI_VERSION == 8                                # two bits and one function: no layout moved
    assert s1 == ctypes.sizeof(ps.Potential) == 32 and s2 == ctypes.sizeof(ps.ProbeSpec) == 56
    assert rc == 1                                                   # PSAMD_ERR_INVALID_ARG


def test_the_new_function_is_declared_exported_and_bound():
    name = "psamd_download_potential_far"
    text = open(os.path.join(ROOT, "include", "psamd.h")).read()
    ps.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", ps.LIB_PATH], check=True, capture_output=True, text=True).stdout
    lib = ps.load()
    assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in the header"
    assert re.search(r" T %s$" % name, exported, re.M), name + " is not exported by the library"
    assert name in [n for n, _, _ in ps.ABI] and getattr(lib, name).restype is ctypes.c_int, name + " is not bound"
    assert lib.psamd_download_potential_far(None, None, 0, None) == 1
    for fn in (ps.ParticleSystem.potential, ps.ParticleSystem.download_potential, ps.ParticleSystem.energy, ps.ParticleSystem.probe):
        assert fn.__defaults__[-1] is False and fn.__code__.co_varnames[:fn.__code__.co_argcount][-1] == "far"


def frame_of(kind, G, n=8192):
    half = G * 2.5 * 0.9995
    xyz = cloud(n, 11, half) if kind == "uniform" else clustered(n, 12, half)
    lists = M.lists_of(xyz, G)
    assert sum(len(l) for l in lists) == n
    return xyz, np.full(n, W, np.float32), lists


@pytest.mark.parametrize("G", [8, 10])
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_the_method_against_the_direct_sum(kind, G):
    xyz, w, lists = frame_of(kind, G)
    pick = np.random.default_rng(13).choice(len(xyz), 400, replace=False)
    cell = M.cells_of(xyz, G)[pick]
    want = F.direct_phi(xyz, w, EPS2, pick)
    dev = lambda got: np.abs(got - want) / np.abs(want)
    near = dev(F.phi64(lists, xyz, w, G, EPS2, xyz[pick], cell, pick, far=False))
    assert np.median(near) > 0.5                                     # (the far part is no small correction)
    for pyramid in (False, True):
        far = dev(F.phi64(lists, xyz, w, G, EPS2, xyz[pick], cell, pick, pyramid=pyramid))
        print("%s cloud, %d bodies on %d^3 cells, %s: far phi median %.3g max %.3g; stencil alone median %.3g max %.3g"
              % (kind, len(xyz), G, "pyramid" if pyramid else "flat", np.median(far), far.max(), np.median(near), near.max()))
        assert np.median(far) < np.median(near)


@pytest.mark.parametrize("pyramid", [False, True], ids=["flat", "pyramid"])
def test_the_two_forms_of_the_model_agree(pyramid):
    """the fp32 association against the fp64 form, both signs of w; a kid among the points (w_eff 0: it sees every body)"""
    G = 8
    xyz, w, lists = frame_of("uniform", G, 4096)
    w = w.copy()
    w[::17] = 0.0
    pick = np.concatenate([np.arange(0, 170, 17), np.random.default_rng(14).choice(len(xyz), 190, replace=False)])
    cell = M.cells_of(xyz, G)[pick]
    for sign in (1.0, -1.0):
        a = F.phi64(lists, xyz, np.float32(sign) * w, G, EPS2, xyz[pick], cell, pick, pyramid=pyramid)
        b = F.phi32(lists, xyz, np.float32(sign) * w, G, EPS2, xyz[pick], cell, pick, pyramid=pyramid)
        rel = np.abs(b - a) / np.abs(a)
        print("%s, sign %+.0f: fp32 association against fp64, max %.3g" % ("pyramid" if pyramid else "flat", sign, rel.max()))
        assert b.dtype == np.float32 and (np.sign(a) == -sign).all() and rel.max() < F.ALLOW


def test_a_confined_cloud_has_no_far_body_and_one_level_is_the_flat_set():
    G = 8
    rng = np.random.default_rng(15)
    xyz = rng.uniform(-4.99, 4.99, (300, 3)).astype(np.float32)      # cells 3..4 on every axis
    w = np.full(300, W, np.float32)
    lists = M.lists_of(xyz, G)
    cell = M.cells_of(xyz, G)
    idx = np.arange(300)
    near = F.phi32(lists, xyz, w, G, EPS2, xyz, cell, idx, far=False)
    for pyramid in (False, True):
        assert np.array_equal(F.phi32(lists, xyz, w, G, EPS2, xyz, cell, idx, pyramid=pyramid), near)
    for c in range(64):
        assert F.far_set(c, 4, True) == F.far_set(c, 4, False)
