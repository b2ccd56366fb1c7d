"""The mass on a lattice without a GPU: the deposit structs of include/psamd.h (psamd_deposit_spec, psamd_deposit_result),
their ctypes mirror and the cross-compiled library agree; the three entry points are declared, exported and bound, NULL
arguments are refused and the ABI is still 8; the definition (tests/deposit_model.py) on hand-worked cases, its mass
conservation and its fp32 form against the plain fp64 form, both within bounds that are derived, not measured."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import deposit_model as D
import particlesystem_amd as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {"psamd_deposit_spec": ps.DepositSpec, "psamd_deposit_result": ps.DepositResult}
NAMES = ("psamd_deposit", "psamd_deposit_result_get", "psamd_download_deposit")


def c_layout(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "psamd.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in py._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    # the entry points have the signatures the mirror binds
    lines.append("int (*f)(psamd_ctx *, const psamd_deposit_spec *) = psamd_deposit; (void)f;")
    lines.append("int (*g)(psamd_ctx *, psamd_deposit_result *) = psamd_deposit_result_get; (void)g;")
    lines.append("int (*h)(psamd_ctx *, int32_t, float *, int64_t, psamd_deposit_result *) = psamd_download_deposit; (void)h;")
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-c", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "layout_c.o")], check=True)      # the header is C as well as C++
    subprocess.run(["g++", "-x", "c++", "-std=c++17", "-Wall", "-Werror", "-c", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "layout.o")], check=True)
    subprocess.run(["g++", str(tmp_path / "layout.o"), "-L" + os.path.dirname(ps.LIB_PATH), "-lpsamd",
                    "-Wl,-rpath," + os.path.dirname(ps.LIB_PATH), "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {tuple(l.split()[:2]): int(l.split()[2]) for l in out.splitlines()}


def test_deposit_structs_match_the_ctypes_mirror(tmp_path):
    ps.build()
    got = c_layout(tmp_path)
    for cname, py in STRUCTS.items():
        assert got[(cname, "sizeof")] == ctypes.sizeof(py), cname
        for field, _ in py._fields_:
            assert got[(cname, field)] == getattr(py, field).offset, (cname, field)
    assert got[("psamd_deposit_result", "sizeof")] == 40 and got[("psamd_deposit_spec", "sizeof")] == 32
    assert [n for n, _ in ps.DepositResult._fields_] == list(D.RESULT_KEYS)


def test_the_mirror_binds_the_three_entry_points_and_the_abi_is_still_8():
    text = open(os.path.join(ROOT, "include", "psamd.h")).read()
    assert int(re.search(r"#define PSAMD_ABI_VERSION (\d+)", text).group(1)) == 8 == ps.ABI_VERSION
    assert "/* ---- mass on a lattice" in text and text.index("/* ---- the field at chosen points") < text.index("/* ---- mass on a lattice")
    names = [n for n, _, _ in ps.ABI]
    for name in NAMES:
        assert re.search(r"^int %s\(psamd_ctx \*ctx, " % name, text, re.M), name + " is not declared"
        assert name in names
    ps.build()
    lib = ps.load()
    assert lib.psamd_abi_version() == 8
    exported = subprocess.run(["nm", "-D", "--defined-only", ps.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r" T %s$" % name, exported, re.M), name + " is not exported"
    invalid = 1                                                              # PSAMD_ERR_INVALID_ARG
    out = np.zeros(8, np.float32)
    assert lib.psamd_deposit(None, None) == invalid
    assert lib.psamd_deposit(None, ctypes.byref(ps.DepositSpec(refine=1))) == invalid
    assert lib.psamd_deposit_result_get(None, None) == invalid
    assert lib.psamd_deposit_result_get(None, ctypes.byref(ps.DepositResult())) == invalid
    assert lib.psamd_download_deposit(None, 1, None, 0, None) == invalid
    assert lib.psamd_download_deposit(None, 1, out.ctypes.data_as(ctypes.c_void_p), 8, None) == invalid
    merged = ps.merge_deposit([dict(voxels=3, bodies=2, skipped=1, mass=1.5, vmax=-math.inf), dict(voxels=5, bodies=0, skipped=0, mass=0.25, vmax=2.0)])
    assert merged == dict(voxels=8, bodies=2, skipped=1, mass=1.75, vmax=2.0)


# ---- the model on hand-worked cases -------------------------------------------------------------------------------------------
# a grid of 4^3 cells of 5 units: the box is [-10, 10)^3; G / 2 = 2

G, CS, CAP = 4, 5.0, 6


def model(xyz, w_eff, refine, exact=False, cell=None, cap=CAP):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    cell = D.locate(xyz[:, 0], xyz[:, 1], xyz[:, 2], G, CS) if cell is None else np.asarray(cell)
    assert (cell >= 0).all()
    x, y, z, w, start, _ = D.frame_of(xyz[:, 0], xyz[:, 1], xyz[:, 2], w_eff, cell, G)
    return D.deposit(x, y, z, w, start, G, CS, cap, refine, exact=exact)


def point(q1, q2, q3):
    """(x, y, z) of cell-axis coordinates: (q1, q2, q3) = (-y, x, -z)"""
    return (q2, -q1, -q3)


@pytest.mark.parametrize("refine", D.REFINES)
def test_a_body_on_a_voxel_centre_gives_that_voxel_its_whole_mass(refine):
    q = D.centres(G, CS, refine)
    M = G * refine
    n1, n2, n3 = 1, M - 2, refine                         # (the centres are multiples of 0.625: exact in fp32)
    r = model([point(q[n1], q[n2], q[n3])], [-48.0], refine)     # the sign of w_eff does not enter
    assert r["rho"][n3, n1, n2] == np.float32(48.0) and np.count_nonzero(r["rho"]) == 1
    assert (r["voxels"], r["bodies"], r["skipped"], r["mass"], r["vmax"]) == (M ** 3, 1, 0, 48.0, 48.0)
    assert r["rho"].dtype == np.float32 and r["rho"].shape == (M, M, M)


@pytest.mark.parametrize("refine", D.REFINES)
def test_a_body_midway_between_eight_centres_gives_an_eighth_each(refine):
    q = D.centres(G, CS, refine)
    n1, n2, n3 = 2, 0, G * refine - 2
    mid = lambda n: 0.5 * (q[n] + q[n + 1])
    r = model([point(mid(n1), mid(n2), mid(n3))], [80.0], refine)
    want = np.zeros_like(r["rho"])
    want[n3:n3 + 2, n1:n1 + 2, n2:n2 + 2] = 10.0
    assert np.array_equal(r["rho"], want) and r["mass"] == 80.0 and r["vmax"] == 10.0


@pytest.mark.parametrize("refine", D.REFINES)
def test_a_body_beyond_the_last_centre_in_a_corner_folds_onto_the_corner_voxel(refine):
    M = G * refine
    hi, lo = np.float32(9.99), np.float32(-9.99)          # within h / 2 of the box faces: past the outermost centres
    r = model([point(hi, hi, hi), point(lo, lo, lo), point(lo, hi, lo)], [7.0, 5.0, 3.0], refine)
    assert r["rho"][M - 1, M - 1, M - 1] == 7.0 and r["rho"][0, 0, 0] == 5.0 and r["rho"][0, 0, M - 1] == 3.0
    assert np.count_nonzero(r["rho"]) == 3 and r["mass"] == 15.0


def test_a_kid_gives_nothing_and_counts_as_a_body():
    # a kid's snapshot entry: the origin, w_eff = 0, in the list of the cell it lives in (here a cell far from the origin's)
    r = model([(0.0, 0.0, 0.0), point(-8.75, -8.75, -8.75)], [0.0, 12.0], 2, cell=[0, 0])      # (-8.75: the centre of voxel 0)
    assert r["bodies"] == 2 and r["skipped"] == 0 and r["mass"] == 12.0 and np.count_nonzero(r["rho"]) == 1
    assert not np.signbit(r["rho"]).any()


def test_a_nan_coordinate_is_skipped_and_counted_once():
    inf = np.float32(np.inf)
    xyz = [(np.nan, 1.0, 1.0), (1.0, inf, 1.0), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0)]
    r = model(xyz, [9.0, 9.0, np.nan, 4.0], 4, cell=[21, 21, 22, 22])
    assert (r["bodies"], r["skipped"]) == (1, 3) and abs(r["mass"] - 4.0) < 4.0 * 2.0 ** -21
    e = model(xyz, [9.0, 9.0, np.nan, 4.0], 4, cell=[21, 21, 22, 22], exact=True)
    assert (e["bodies"], e["skipped"]) == (1, 3)


def test_the_entry_past_the_list_cap_gives_nothing():
    q = D.centres(G, CS, 1)
    xyz = [point(q[1], q[1], q[1])] * (CAP + 2)
    r = model(xyz, np.arange(1, CAP + 3, dtype=np.float32), 1)
    assert r["bodies"] == CAP and r["rho"][1, 1, 1] == sum(range(1, CAP + 1)) == r["mass"]       # 7 and 8 are not bodies


def test_a_body_whose_cell_does_not_fit_its_position_reaches_the_stencil_only():
    # listed in cell (0, 0, 0) but placed two cells along q2: on refine 1 nothing of it lies within one cell
    q = D.centres(G, CS, 1)
    r = model([point(q[0], q[2], q[0])], [5.0], 1, cell=[0])
    assert r["bodies"] == 1 and r["mass"] == 0.0 and not r["rho"].any()
    # midway between the centres of cells 1 and 2 along q2: the half that falls on cell 1 stays
    r = model([point(q[0], 0.5 * (q[1] + q[2]), q[0])], [6.0], 1, cell=[0])
    assert r["rho"][0, 0, 1] == 3.0 and r["mass"] == 3.0


# ---- derived bounds ------------------------------------------------------------------------------------------------------------

def cloud(n, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-10.0, 10.0, (n, 3)).astype(np.float32)
    xyz = xyz[(np.abs(xyz) < 10.0).all(1)]
    return xyz, rng.uniform(1.0, 100.0, len(xyz)).astype(np.float32)


@pytest.mark.parametrize("refine", D.REFINES)
def test_the_model_conserves_mass_and_agrees_with_the_fp64_form(refine):
    xyz, w = cloud(3000, 7 + refine)
    a = model(xyz, w, refine, cap=10 ** 6)
    b = model(xyz, w, refine, exact=True, cap=10 ** 6)
    total = math.fsum(float(v) for v in w)
    # a body's weights per axis add to 1 up to RN(1 - f): 2^-24; the three products round once each: four roundings of 2^-24
    # at the most on any term, and the terms are non-negative: 4 * 2^-24 < 2^-21 relative on their sum
    assert abs(a["mass"] - total) <= 2.0 ** -21 * total, (a["mass"], total)
    assert abs(b["mass"] - total) <= 2.0 ** -50 * total
    # u = RN(RN(s inv_h) + off).  M is a power of two here and, off the clamped rim (where the weights do not move), |u| < M and
    # |t| < M / 2: u's rounding is at most M 2^-25, t's M 2^-26, and inv_h's own 2^-25 relative of |t| another M 2^-26 -- u is
    # within M 2^-24 of the exact one.  A trilinear weight moves by at most that per axis (the clamp and the fold are
    # 1-Lipschitz), a term by at most 3 M 2^-24 m, and its own four roundings add 4 * 2^-24 m <= M 2^-24 m (M >= 4)
    M = G * refine
    bound = 4.0 * M * 2.0 ** -24 * b["support"]
    err = np.abs(a["sums"] - b["sums"])
    print("refine %d: largest |fp32 - fp64| / bound %.3g" % (refine, (err[bound > 0] / bound[bound > 0]).max()))
    assert (err <= bound).all()
    assert (a["sums"][b["support"] == 0] == 0).all()
