"""Changing particles in place without a GPU: the update structs of include/psamd.h (psamd_update_spec,
psamd_update_result), their ctypes mirror and the cross-compiled library agree; the two entry points are declared,
exported and bound, and the ABI is still 8; the serial definition (tests/update_model.py) on hand-worked cases."""
import ctypes
import os
import re
import subprocess

import numpy as np

import particlesystem_amd as ps
import update_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {"psamd_update_spec": ps.Update, "psamd_update_result": ps.UpdateResult}
BITS = ("VEL", "AGE", "MASS", "FERT", "ADD", "EXPORT_ORDER")


def c_layout(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "psamd.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in py._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    for b in BITS:
        lines.append('printf("bit %s %%u\\n", PSAMD_UPDATE_%s);' % (b, b))
    # the entry points have the signatures the mirror binds
    lines.append("int (*f)(psamd_ctx *, const psamd_update_spec *) = psamd_update; (void)f;")
    lines.append("int (*g)(psamd_ctx *, psamd_update_result *) = psamd_update_result_get; (void)g;")
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


def test_update_structs_match_the_ctypes_mirror(tmp_path):
    ps.build()
    got = c_layout(tmp_path)
    for cname, py in STRUCTS.items():
        assert got[(cname, "sizeof")] == ctypes.sizeof(py), cname
        for field, _ in py._fields_:
            assert got[(cname, field)] == getattr(py, field).offset, (cname, field)
    assert got[("psamd_update_spec", "sizeof")] == 72 and got[("psamd_update_result", "sizeof")] == 48
    assert [n for n, _ in ps.UpdateResult._fields_] == list(M.RESULT_KEYS)
    want = dict(VEL=0x1, AGE=0x2, MASS=0x4, FERT=0x8, ADD=0x100, EXPORT_ORDER=0x200)
    for b in BITS:
        assert got[("bit", b)] == want[b] == getattr(ps, "UPDATE_" + b) == getattr(M, b), b
    assert (ps.UPDATED, ps.UPDATE_NOT_LIVE, ps.UPDATE_FOREIGN, ps.UPDATE_INVALID, ps.UPDATE_DUPLICATE) == \
           (M.UPDATED, M.NOT_LIVE, M.FOREIGN, M.INVALID, M.DUPLICATE) == (0, 1, 2, 3, 4)


def test_the_mirror_binds_both_entry_points_and_the_abi_is_still_8():
    text = open(os.path.join(ROOT, "include", "psamd.h")).read()
    assert int(re.search(r"#define PSAMD_ABI_VERSION (\d+)", text).group(1)) == 8 == ps.ABI_VERSION
    for name in ("psamd_update", "psamd_update_result_get"):
        assert re.search(r"^int %s\(psamd_ctx \*ctx, " % name, text, re.M), name + " is not declared"
    names = [n for n, _, _ in ps.ABI]
    assert "psamd_update" in names and "psamd_update_result_get" in names
    ps.build()
    lib = ps.load()
    assert lib.psamd_abi_version() == 8
    exported = subprocess.run(["nm", "-D", "--defined-only", ps.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r" T psamd_update$", exported, re.M) and re.search(r" T psamd_update_result_get$", exported, re.M)
    assert lib.psamd_update(None, None) == 1 and lib.psamd_update_result_get(None, None) == 1     # PSAMD_ERR_INVALID_ARG
    assert lib.psamd_update(None, ctypes.byref(ps.Update(fields=ps.UPDATE_VEL))) == 1


# ---- the model on hand-worked cases -------------------------------------------------------------------------------------------

def container():
    """eight slots of a grid of 27 cells: 0, 1, 2, 5, 7 live; 3 free; 4 mid-step (cell <= -2); 6 a cell past the grid"""
    p = np.zeros(8, ps.P_DTYPE)
    p["id"] = np.arange(8)
    p["cell"] = [3, 0, 26, -1, -7, 9, 27, 12]
    for k, f in enumerate(("w", "age", "fertility_age", "x", "y", "z", "vx", "vy", "vz", "ax", "ay", "az")):
        p[f] = 100.0 * (k + 1) + np.arange(8)
    return p


def changed(a, b):
    """{(slot, field)} whose bytes differ"""
    return {(int(s), f) for f in a.dtype.names for s in np.nonzero(a[f].view(np.uint8 if a[f].dtype.itemsize == 1 else np.uint32)
                                                                   != b[f].view(np.uint8 if b[f].dtype.itemsize == 1 else np.uint32))[0]}


def test_a_duplicate_a_free_slot_and_both_ends_of_the_range():
    p = container()
    ids = np.array([5, 3, 5, 0, 7, -1, 8, 4, 6, 0], np.int32)
    vel4 = (np.arange(40, dtype=np.float32) + 0.5).reshape(10, 4)
    q, out, res = M.apply(p, 27, M.VEL | M.AGE, ids=ids, vel4=vel4)
    #                      5  3  5  0  7 -1  8  4  6  0
    assert out.tolist() == [0, 1, 4, 0, 0, 3, 3, 1, 1, 4]
    assert res == dict(done=10, updated=3, not_live=3, foreign=0, invalid=2, duplicate=2)
    assert changed(p, q) == {(s, f) for s in (5, 0, 7) for f in ("vx", "vy", "vz", "age")}
    # the first occurrence wins: slot 5 holds entry 0, slot 0 entry 3 -- not entries 2 and 9
    assert [q[f][5] for f in ("vx", "vy", "vz", "age")] == [0.5, 1.5, 2.5, 3.5]
    assert [q[f][0] for f in ("vx", "vy", "vz", "age")] == [12.5, 13.5, 14.5, 15.5]
    assert [q[f][7] for f in ("vx", "vy", "vz", "age")] == [16.5, 17.5, 18.5, 19.5]
    # a count: the first three entries only; a slab that does not own slots 4 .. 7
    q, out, res = M.apply(p, 27, M.MASS | M.FERT, ids=ids, w=vel4[:, 0].copy(), fert_age=vel4[:, 1].copy(), n=3,
                          owned=np.arange(8) < 4)
    assert out.tolist() == [2, 1, 2] and res == dict(done=3, updated=0, not_live=1, foreign=2, invalid=0, duplicate=0)
    assert q.tobytes() == p.tobytes()


def test_add_is_one_fp32_addition_that_rounds():
    p = container()
    p["vx"][1], p["vy"][1], p["vz"][1] = 1.0, 16777216.0, -0.1
    kick = np.array([[2.0 ** -24, 1.0, 0.3, 99.0]], np.float32)
    q, out, res = M.apply(p, 27, M.VEL | M.ADD, ids=np.array([1], np.int32), vel4=kick)
    assert out.tolist() == [0] and res["updated"] == 1
    # 1 + 2^-24 is a tie and rounds to the even 1; 2^24 + 1 is a tie and rounds to the even 2^24; -0.1f + 0.3f rounds once
    assert q["vx"][1] == np.float32(1.0) and q["vy"][1] == np.float32(16777216.0)
    exact = float(np.float32(-0.1)) + float(np.float32(0.3))
    assert q["vz"][1] == np.float32(exact) and float(q["vz"][1]) != exact
    assert changed(p, q) <= {(1, "vz")} and q["age"][1] == p["age"][1]       # ADD reads no age


def test_export_order_and_set_keeps_the_bits():
    p = container()
    words = np.array([0x7fc00001, 0xffc12345, 0x80000000, 0x7f800000, 0x00000001, 0xff800000, 0x7fa00000], np.uint32)
    vel4 = np.zeros((7, 4), np.float32)
    vel4.view(np.uint32)[:, 0] = words
    vel4.view(np.uint32)[:, 2] = words[::-1]
    q, out, res = M.apply(p, 27, M.VEL, vel4=vel4)
    # the live slots in ascending id are 0, 1, 2, 5, 7: entries 5 and 6 find no particle
    assert out.tolist() == [0, 0, 0, 0, 0, 1, 1] and res == dict(done=7, updated=5, not_live=2, foreign=0, invalid=0, duplicate=0)
    assert q["vx"].view(np.uint32)[[0, 1, 2, 5, 7]].tolist() == words[:5].tolist()
    assert q["vz"].view(np.uint32)[[0, 1, 2, 5, 7]].tolist() == words[::-1][:5].tolist()
    assert changed(p, q) <= {(s, f) for s in (0, 1, 2, 5, 7) for f in ("vx", "vy", "vz")}
    # n below the live count: the live particles past n are left alone
    q, out, res = M.apply(p, 27, M.AGE, vel4=vel4, n=2)
    assert out.tolist() == [0, 0] and changed(p, q) == {(0, "age"), (1, "age")}
