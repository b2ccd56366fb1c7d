"""A lattice field at the particles without a GPU: the sample structs of include/psamd.h (psamd_sample_spec,
psamd_sample_result), their ctypes mirror and the cross-compiled library agree; the two entry points are declared, exported and
bound, NULL arguments are refused and the ABI is still 8; the definition (tests/sample_model.py) on hand-worked cases; and the
adjointness of the two models -- deposit_model spreads with the weights sample_model reads with -- within a derived bound."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import deposit_model as D
import particlesystem_amd as ps
import sample_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {"psamd_sample_spec": ps.SampleSpec, "psamd_sample_result": ps.SampleResult}
NAMES = ("psamd_sample", "psamd_sample_result_get")


def c_layout(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "psamd.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in py._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    # the entry points have the signatures the mirror binds, the flags their values
    lines.append("int (*f)(psamd_ctx *, const psamd_sample_spec *) = psamd_sample; (void)f;")
    lines.append("int (*g)(psamd_ctx *, psamd_sample_result *) = psamd_sample_result_get; (void)g;")
    lines.append('printf("flags vec4 %u\\nflags order %u\\n", PSAMD_SAMPLE_VEC4, PSAMD_SAMPLE_EXPORT_ORDER);')
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


def test_sample_structs_match_the_ctypes_mirror(tmp_path):
    ps.build()
    got = c_layout(tmp_path)
    for cname, py in STRUCTS.items():
        assert got[(cname, "sizeof")] == ctypes.sizeof(py), cname
        for field, _ in py._fields_:
            assert got[(cname, field)] == getattr(py, field).offset, (cname, field)
    assert got[("psamd_sample_spec", "sizeof")] == 80 and got[("psamd_sample_result", "sizeof")] == 32
    assert [n for n, _ in ps.SampleResult._fields_] == list(S.RESULT_KEYS)
    assert (got[("flags", "vec4")], got[("flags", "order")]) == (ps.SAMPLE_VEC4, ps.SAMPLE_EXPORT_ORDER) == (1, 2)


def test_the_mirror_binds_the_two_entry_points_and_the_abi_is_still_8():
    text = open(os.path.join(ROOT, "include", "psamd.h")).read()
    assert int(re.search(r"#define PSAMD_ABI_VERSION (\d+)", text).group(1)) == 8 == ps.ABI_VERSION
    assert text.index("/* ---- mass on a lattice") < text.index("/* ---- a lattice field at the particles") < text.index("/* ---- long-range gravity")
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
    assert lib.psamd_sample(None, None) == invalid
    assert lib.psamd_sample(None, ctypes.byref(ps.SampleSpec(refine=1))) == invalid
    assert lib.psamd_sample_result_get(None, None) == invalid
    assert lib.psamd_sample_result_get(None, ctypes.byref(ps.SampleResult())) == invalid
    merged = ps.merge_sample([dict(done=5, served=3, outside=2, nonfinite=1), dict(done=4, served=4, outside=0, nonfinite=0)])
    assert merged == dict(done=9, served=7, outside=2, nonfinite=1)


# ---- the model on hand-worked cases -------------------------------------------------------------------------------------------
# test_deposit_cpu.py's grid of 4^3 cells of 5 units: the box is [-10, 10)^3; G / 2 = 2

G, CS = 4, 5.0


def point(q1, q2, q3):
    """(x, y, z) of cell-axis coordinates: (q1, q2, q3) = (-y, x, -z)"""
    return (q2, -q1, -q3)


def field_of(refine, seed, vec4=False):
    M = G * refine
    return np.random.default_rng(seed).standard_normal((M, M, M, 4) if vec4 else (M, M, M)).astype(np.float32)


def model(points, field, scale=1.0):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    return S.sample(p[:, 0], p[:, 1], p[:, 2], field, G, CS, scale)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("refine", D.REFINES)
def test_a_point_on_a_voxel_centre_returns_the_voxel_whatever_its_neighbours_hold(refine):
    q = D.centres(G, CS, refine)                              # (multiples of 0.625: exact in fp32)
    M = G * refine
    for vec4 in (False, True):
        F = field_of(refine, 5 + refine, vec4)
        n1, n2, n3 = 1, M - 2, refine
        keep = F[n3, n1, n2].copy()
        F[n3 - 1:n3 + 2, n1 - 1:n1 + 2, n2 - 1:n2 + 2] = np.nan                # all 26 neighbours, and ...
        F[n3, n1, n2] = keep                                                   # ... not the voxel
        F[0, 0, 0] = -0.0
        out, oc, res, _ = model([point(q[n1], q[n2], q[n3]), point(q[0], q[0], q[0])], F)
        assert np.array_equal(bits(out[0]), bits(keep)) and (bits(out[1]) == 0).all(), "-0 becomes +0"
        assert list(oc) == [0, 0] and res == dict(done=2, served=2, outside=0, nonfinite=0)
        assert out.dtype == np.float32 and out.shape == ((2, 4) if vec4 else (2,))


@pytest.mark.parametrize("refine", D.REFINES)
def test_a_point_midway_between_eight_centres_returns_the_rounded_mean(refine):
    q = D.centres(G, CS, refine)
    n1, n2, n3 = 2, 0, G * refine - 2
    mid = lambda n: 0.5 * (q[n] + q[n + 1])
    F = field_of(refine, 9 + refine)
    out, _, _, Sk = model([point(mid(n1), mid(n2), mid(n3))], F)
    eight = F[n3:n3 + 2, n1:n1 + 2, n2:n2 + 2].astype(np.float64)
    assert out[0] == np.float32(eight.sum() / 8.0) and Sk[0] == np.abs(eight).sum() / 8.0       # (eighths and their fp64 sum: exact)


@pytest.mark.parametrize("refine", D.REFINES)
def test_a_point_beyond_the_last_centre_in_a_corner_returns_the_corner_voxel(refine):
    M = G * refine
    hi, lo = np.float32(9.99), np.float32(-9.99)
    F = field_of(refine, 13 + refine)
    F[1:M - 1, 1:M - 1, 1:M - 1] = np.nan
    out, oc, _, _ = model([point(hi, hi, hi), point(lo, lo, lo), point(lo, hi, lo)], F)
    assert np.array_equal(bits(out), bits([F[M - 1, M - 1, M - 1], F[0, 0, 0], F[0, 0, M - 1]])) and (oc == 0).all()


def test_outside_the_box_and_coordinates_that_are_no_numbers():
    F = field_of(2, 17, vec4=True)
    inf = np.float32(np.inf)
    pts = [(10.0, 0.0, 0.0), (0.0, 10.0001, 0.0), (0.0, 0.0, -10.5), (np.nan, 1.0, 1.0), (1.0, inf, 1.0), (1.0, 1.0, -inf), (1e30, 0.0, 0.0),
           (-10.0, 10.0, 10.0), (1.0, 1.0, 1.0)]
    out, oc, res, Sk = model(pts, F)
    # x = 10 is the first point past the box along q2; (x, y, z) = (-10, 10, 10) is cell (0, 0, 0)'s corner: inside
    assert list(oc) == [1] * 7 + [0, 0] and res == dict(done=9, served=2, outside=7, nonfinite=0)
    assert (bits(out[:7]) == S.QNAN).all() and np.isfinite(out[7:]).all() and (Sk[:7] == 0).all()
    F[:] = np.nan
    assert model(pts, F)[2] == dict(done=9, served=2, outside=7, nonfinite=2)


def test_scale_is_applied_once_after_the_rounding_to_float():
    rng = np.random.default_rng(23)
    pts = rng.uniform(-9.9, 9.9, (400, 3)).astype(np.float32)
    F = field_of(2, 29)
    one = model(pts, F)[0]
    three = model(pts, F, scale=3.0)[0]
    assert np.array_equal(bits(three), bits(np.float32(3.0) * one))
    # ... which is not the rounding of three times the fp64 sum: some of 400 entries round twice to another float
    x, y, z = pts.T
    ax = [D._axis32(s, G, CS, 2) for s in (-y, x, -z)]
    sums = np.zeros(400)
    for d3 in (0, 1):
        for d1 in (0, 1):
            for d2 in (0, 1):
                W = (ax[0][1 + d1] * ax[1][1 + d2]) * ax[2][1 + d3]
                idx = (np.minimum(ax[2][0] + d3, 7) * 8 + np.minimum(ax[0][0] + d1, 7)) * 8 + np.minimum(ax[1][0] + d2, 7)
                sums += (W * F.ravel()[idx]).astype(np.float64)
    assert np.array_equal(bits(sums.astype(np.float32)), bits(one))
    assert (bits((3.0 * sums).astype(np.float32)) != bits(three)).any()
    assert (bits(model(pts, F, scale=0.0)[0]) << 1 == 0).all()                 # scale 0: zeros (of either sign)


# ---- adjointness of the two models ---------------------------------------------------------------------------------------------
# sum_v F_v rho_v = sum_b m_b sample_b up to rounding.  The two sides share every W; a deposit term RN(W m) and a sample term
# RN(W F) take one fp32 rounding each beyond it, every voxel (rho) and every sample one final rounding to float: four units of
# 2^-24 on sum_b m_b S_b, S_b = sum_v W_bv |F_v|; the fifth covers second-order terms and the fp64 chains.

def adjoint_case(Gn, refine, seed=3):
    xyz = S.rough_points(Gn, CS, seed)
    rng = np.random.default_rng(seed + 100)
    w = rng.uniform(20.0, 100.0, len(xyz)).astype(np.float32)
    w[::29] = 0.0                                            # massless bodies stay; no clump, no kids, nothing skipped
    M = Gn * refine
    F = rng.standard_normal((M, M, M)).astype(np.float32)
    return xyz, w, F


@pytest.mark.parametrize("refine", D.REFINES)
@pytest.mark.parametrize("Gn", [8, 9])
def test_the_sample_is_the_adjoint_of_the_deposit(Gn, refine):
    xyz, w, F = adjoint_case(Gn, refine)
    cell = D.locate(xyz[:, 0], xyz[:, 1], xyz[:, 2], Gn, CS)
    assert (cell >= 0).all()
    x, y, z, ws, start, order = D.frame_of(xyz[:, 0], xyz[:, 1], xyz[:, 2], w, cell, Gn)
    dep = D.deposit(x, y, z, ws, start, Gn, CS, 10 ** 6, refine)
    assert dep["bodies"] == len(xyz) and dep["skipped"] == 0
    smp, oc, res, Sk = S.sample(xyz[:, 0], xyz[:, 1], xyz[:, 2], F, Gn, CS)
    assert res["served"] == len(xyz) and (oc == 0).all()
    m = np.abs(w)
    for name, lattice in (("sums", dep["sums"]), ("rho", dep["rho"])):
        err, scale = S.adjoint_sides(F, lattice, m, smp, Sk)
        print("%d^3 cells, refine %d, %s: |difference| / (2^-24 sum m S) = %.3g" % (Gn, refine, name, err / (2.0 ** -24 * scale)))
        assert err <= 5.0 * 2.0 ** -24 * scale, (name, err, scale)
