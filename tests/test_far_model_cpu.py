"""The far field without a GPU, what is one for all five features (far monopoles, the pyramid, quadrupoles, the far potential
and probes, and those on quadrupole contexts): the header, the ctypes mirror and the library agree on a feature's flag or bits and
on its entry points -- one test over the FEATURES table, each row with its C snippet, expected values and names --; and the model
(far_model.py) computes what the files it replaced computed (tests/golden/far_model.json: the four method files;
tests/golden/far_field_quadrupole.json: the quadrupole field's own file; both written by scripts/far_model_golden.py from those files as
git has them).  far_model.py is the oracle of every GPU far-field test, so a silent change to it would weaken them all.  What
one method has -- its caps against the direct sum, its hand-made frames -- is in its test_far_*_cpu.py."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import far_model as F
import particlesystem_amd as ps
from far_harness import INVALID_ARG, ROOT, c_prints, declared_exported_bound

sys.path.insert(0, os.path.join(ROOT, "scripts"))

import far_model_golden  # noqa: E402


# ---- 1. the C surface of the five features -------------------------------------------------------------------------------------

def monopole_values(flag, clash, abi):
    assert flag == ps.FLAG_FAR_MONOPOLE == 0x10 and clash == 0
    assert abi == ps.ABI_VERSION == 8                                # one flag bit and one function: no layout moved


def pyramid_values(flag, clash, abi, r1, r2):
    assert flag == ps.FLAG_FAR_PYRAMID == 0x20 and clash == 0
    assert abi == ps.ABI_VERSION == 8                                # one flag bit and two functions: no layout moved
    assert r1 == 1 and r2 == 1                                       # PSAMD_ERR_INVALID_ARG


def quadrupole_values(flag, clash, abi, r):
    assert flag == ps.FLAG_FAR_QUADRUPOLE == 0x40 and clash == 0
    others = [getattr(ps, n) for n in dir(ps) if n.startswith("FLAG_") and n != "FLAG_FAR_QUADRUPOLE"]
    assert len(others) >= 6 and not any(ps.FLAG_FAR_QUADRUPOLE & o for o in others)
    assert abi == ps.ABI_VERSION == 8                                # one flag bit and one function: no layout moved
    assert r == 1                                                    # PSAMD_ERR_INVALID_ARG


def potential_values(pot, prb, clash, abi, rc, s1, s2):
    assert pot == ps.POTENTIAL_FAR == 0x1 and prb == ps.PROBE_FAR == 0x4 and clash == 0
    assert abi == ps.ABI_VERSION == 8                                # two bits and one function: no layout moved
    assert s1 == ctypes.sizeof(ps.Potential) == 32 and s2 == ctypes.sizeof(ps.ProbeSpec) == 56
    assert rc == 1                                                   # PSAMD_ERR_INVALID_ARG


def quadrupole_field_values(*got):
    assert list(got) == [0x2, 0x8, 0, 0, 8, 32, 56, 8, INVALID_ARG]  # the two bits clash with none; no layout moved
    assert (ps.POTENTIAL_QUADRUPOLE, ps.PROBE_QUADRUPOLE) == (0x2, 0x8)


def monopole_bound(lib):
    assert lib.psamd_download_cell_moments(None, None) == 1          # PSAMD_ERR_INVALID_ARG
    assert callable(ps.ParticleSystem.download_cell_moments)


def pyramid_bound(lib):
    assert lib.psamd_far_levels(None, None, None) == 1               # PSAMD_ERR_INVALID_ARG
    assert lib.psamd_download_level_moments(None, 0, None) == 1
    assert callable(ps.ParticleSystem.download_level_moments) and callable(ps.far_levels)


def quadrupole_bound(lib):
    assert lib.psamd_download_level_quadrupoles(None, 0, None) == 1  # PSAMD_ERR_INVALID_ARG
    out = (ctypes.c_float * 6)()
    assert lib.psamd_download_level_quadrupoles(None, 0, out) == 1
    assert callable(ps.ParticleSystem.download_level_quadrupoles)


def potential_bound(lib):
    assert lib.psamd_download_potential_far(None, None, 0, None) == 1
    for fn in (ps.ParticleSystem.potential, ps.ParticleSystem.download_potential, ps.ParticleSystem.energy, ps.ParticleSystem.probe):
        assert fn.__defaults__[-1] is False and fn.__code__.co_varnames[:fn.__code__.co_argcount][-1] == "far"


def quadrupole_field_bound(lib):
    assert lib.psamd_download_potential_flags(None, ps.POTENTIAL_FAR | ps.POTENTIAL_QUADRUPOLE, None, 0, None) == INVALID_ARG
    assert lib.psamd_download_potential_flags(None, 0, None, 0, None) == INVALID_ARG


# feature: (the body of a C main() that prints integers, what they must be, the entry points, what calling them unbound gives)
FEATURES = {
    "monopole": (
        'int (*f)(psamd_ctx *, void *) = psamd_download_cell_moments; (void)f;\n'
        'printf("%u %u %d\\n", PSAMD_FLAG_FAR_MONOPOLE, PSAMD_FLAG_FAR_MONOPOLE & (PSAMD_FLAG_EXPLOSIONS | PSAMD_FLAG_FAST_MATH | '
        'PSAMD_FLAG_ALL_PAIRS | PSAMD_FLAG_EULER), psamd_abi_version());\n',
        monopole_values, ("psamd_download_cell_moments",), monopole_bound),
    "pyramid": (
        'int (*f)(const psamd_config *, int32_t *, int32_t *) = psamd_far_levels; (void)f;\n'
        'int (*g)(psamd_ctx *, int32_t, void *) = psamd_download_level_moments; (void)g;\n'
        'int32_t n = 0, dims[16];\n'
        'printf("%u %u %d %d %d\\n", PSAMD_FLAG_FAR_PYRAMID, PSAMD_FLAG_FAR_PYRAMID & (PSAMD_FLAG_EXPLOSIONS | PSAMD_FLAG_FAST_MATH | '
        'PSAMD_FLAG_ALL_PAIRS | PSAMD_FLAG_EULER | PSAMD_FLAG_FAR_MONOPOLE), psamd_abi_version(), '
        'psamd_far_levels(NULL, &n, dims), psamd_download_level_moments(NULL, 0, dims));\n',
        pyramid_values, ("psamd_far_levels", "psamd_download_level_moments"), pyramid_bound),
    "quadrupole": (
        'int (*g)(psamd_ctx *, int32_t, void *) = psamd_download_level_quadrupoles; (void)g;\n'
        'float out[6];\n'
        'printf("%u %u %d %d\\n", PSAMD_FLAG_FAR_QUADRUPOLE, PSAMD_FLAG_FAR_QUADRUPOLE & (PSAMD_FLAG_EXPLOSIONS | '
        'PSAMD_FLAG_FAST_MATH | PSAMD_FLAG_ALL_PAIRS | PSAMD_FLAG_EULER | PSAMD_FLAG_FAR_MONOPOLE | PSAMD_FLAG_FAR_PYRAMID), '
        'psamd_abi_version(), psamd_download_level_quadrupoles(NULL, 0, out));\n',
        quadrupole_values, ("psamd_download_level_quadrupoles",), quadrupole_bound),
    "potential": (
        'int (*f)(psamd_ctx *, float *, int64_t, psamd_potential_result *) = psamd_download_potential_far; (void)f;\n'
        'printf("%u %u %u %d %d %zu %zu\\n", PSAMD_POTENTIAL_FAR, PSAMD_PROBE_FAR, PSAMD_PROBE_FAR & (PSAMD_PROBE_ACC | PSAMD_PROBE_PHI), '
        'psamd_abi_version(), psamd_download_potential_far(NULL, NULL, 0, NULL), sizeof(psamd_potential_spec), sizeof(psamd_probe_spec));\n',
        potential_values, ("psamd_download_potential_far",), potential_bound),
    "quadrupole_field": (
        'printf("%u %u %u %u %d %zu %zu\\n", PSAMD_POTENTIAL_QUADRUPOLE, PSAMD_PROBE_QUADRUPOLE, '
        'PSAMD_POTENTIAL_QUADRUPOLE & PSAMD_POTENTIAL_FAR, '
        'PSAMD_PROBE_QUADRUPOLE & (PSAMD_PROBE_ACC | PSAMD_PROBE_PHI | PSAMD_PROBE_FAR), PSAMD_ABI_VERSION, '
        'sizeof(psamd_potential_spec), sizeof(psamd_probe_spec));\n'
        'printf("%d %d\\n", psamd_abi_version(), psamd_download_potential_flags(NULL, PSAMD_POTENTIAL_FAR | PSAMD_POTENTIAL_QUADRUPOLE, NULL, 0, NULL));\n',
        quadrupole_field_values, ("psamd_download_potential_flags",), quadrupole_field_bound),
}


@pytest.mark.parametrize("feature", list(FEATURES))
def test_header_mirror_and_library_agree(feature, tmp_path):
    body, values, _, _ = FEATURES[feature]
    values(*c_prints(tmp_path, body))


@pytest.mark.parametrize("feature", list(FEATURES))
def test_the_new_symbols_are_declared_exported_and_bound(feature):
    _, _, names, bound = FEATURES[feature]
    bound(declared_exported_bound(names))


# ---- 2. the model is the one it replaced ---------------------------------------------------------------------------------------

def same_as_golden(file, got, approximate):
    """`got` against the frames of tests/golden/`file`: the same keys, digests and fp64 fields equal bit for bit, the
    `approximate` fields within far_model_golden.NEAR of their norm"""
    with open(os.path.join(ROOT, "tests", "golden", file)) as fi:
        golden = json.load(fi)
    assert len(golden["commit"]) == 40 and golden["commit"] in golden["command"]
    want = golden["frames"]
    assert sorted(got) == sorted(want) and len(want) == len(far_model_golden.FRAMES)
    for name in want:
        for kind in ("sha256", "f64"):
            assert sorted(got[name][kind]) == sorted(want[name][kind])
            differ = sorted(k for k in want[name][kind] if got[name][kind][k] != want[name][kind][k] and k not in approximate)
            assert not differ, "%s: %s differ(s) from what the model computed at commit %s" % (name, ", ".join(differ), golden["commit"][:7])
        for k in approximate:
            a, b = far_model_golden.unpack(got[name]["f64"][k]), far_model_golden.unpack(want[name]["f64"][k])
            print("%s, %s: %.3g of the norm from the golden file" % (name, k, np.linalg.norm(a - b) / np.linalg.norm(b)))
            assert a.shape == b.shape and np.linalg.norm(a - b) <= far_model_golden.NEAR * np.linalg.norm(b) > 0, (name, k)


def test_the_model_is_the_parents():
    """far_model.py computes what the four files it replaced computed at the commit tests/golden/far_model.json names
    (scripts/far_model_golden.py wrote it from them): the digests are equal, and so are the fp64 fields, bit for bit -- the order
    of bodies in every sum was kept.  The two fields with the quadrupole term are held to far_model_golden.NEAR of their norm
    instead (they came out bit-equal where the file was written; far_model_golden.py says why that may not hold elsewhere)"""
    same_as_golden("far_model.json", far_model_golden.quantities(F), far_model_golden.APPROXIMATE)


def test_the_quadrupole_field_is_the_parents():
    """far_model.py's phi64, phi32, accel64 and quad_sum64 of the quadrupole method compute what the field's own model file computed on
    the far_model.py of the commit tests/golden/far_field_quadrupole.json names: phi32's digest is equal; the three fp64 fields
    hold a float64 power and are held to far_model_golden.NEAR of their norm (they came out bit-equal where the file was written)"""
    same_as_golden("far_field_quadrupole.json", far_model_golden.field_quantities(F), far_model_golden.FIELD_APPROXIMATE)
