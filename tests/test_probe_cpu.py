"""The probe structs of include/psamd.h (psamd_probe_spec, psamd_probe_result) and their ctypes mirror agree: a small C
program compiled against the header prints sizeof / offsetof of every member, the mirror's layout must match; the two
entry points are declared, exported and bound, and refuse null arguments; merge_probe on hand-made records; the header
still says ABI 8 (the feature adds entry points and structs, no layout moves)."""
import ctypes
import os
import re
import subprocess

import numpy as np

import particlesystem_amd as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {"psamd_probe_spec": "ProbeSpec", "psamd_probe_result": "ProbeResult"}
ENTRY_POINTS = ("psamd_probe", "psamd_probe_result_get")


def c_layout(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "psamd.h"', "int main(void) {"]
    for cname, pyname in STRUCTS.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in getattr(ps, pyname)._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines.append('printf("bits acc %u\\n", PSAMD_PROBE_ACC); printf("bits phi %u\\n", PSAMD_PROBE_PHI);')
    # the entry points have the signatures the mirror binds
    lines.append("int (*f)(psamd_ctx *, const psamd_probe_spec *) = psamd_probe; (void)f;")
    lines.append("int (*g)(psamd_ctx *, psamd_probe_result *) = psamd_probe_result_get; (void)g;")
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


def test_probe_structs_match_the_ctypes_mirror(tmp_path):
    ps.build()
    got = c_layout(tmp_path)
    for cname, pyname in STRUCTS.items():
        py = getattr(ps, pyname)
        assert got[(cname, "sizeof")] == ctypes.sizeof(py), cname
        for field, _ in py._fields_:
            assert got[(cname, field)] == getattr(py, field).offset, (cname, field)
    assert got[("psamd_probe_result", "sizeof")] == 40 and got[("psamd_probe_spec", "sizeof")] == 56
    assert got[("bits", "acc")] == ps.PROBE_ACC == 1 and got[("bits", "phi")] == ps.PROBE_PHI == 2


def test_the_two_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "psamd.h")).read()
    names = [n for n, _, _ in ps.ABI]
    ps.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", ps.LIB_PATH], check=True, capture_output=True, text=True).stdout
    lib = ps.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in the header"
        assert re.search(r" T %s$" % name, exported, re.M), name + " is not exported by the library"
        assert name in names and getattr(lib, name).restype is ctypes.c_int, name + " is not bound"


def test_null_arguments_are_refused():
    ps.build()
    lib = ps.load()
    assert lib.psamd_probe(None, None) == 1                          # PSAMD_ERR_INVALID_ARG
    assert lib.psamd_probe(None, ctypes.byref(ps.ProbeSpec(fields=3))) == 1
    assert lib.psamd_probe_result_get(None, None) == 1
    assert lib.psamd_probe_result_get(None, ctypes.byref(ps.ProbeResult())) == 1


def test_merge_probe_takes_each_entry_from_the_rank_that_served_it():
    nan = np.float32(np.nan)
    # four entries: rank 0 serves entry 0, rank 1 entries 1 and 3, entry 2 is outside the box for both
    a = {"out4": np.array([[1, 2, 3, 4], [nan] * 4, [nan] * 4, [nan] * 4], np.float32), "outcome": np.array([0, 2, 1, 2], np.int32),
         "done": 4, "served": 1, "outside": 1, "foreign": 2, "nonfinite": 0}
    b = {"out4": np.array([[nan] * 4, [5, 6, 7, 8], [nan] * 4, [9, np.inf, 0, -1]], np.float32), "outcome": np.array([2, 0, 1, 0], np.int32),
         "done": 4, "served": 2, "outside": 1, "foreign": 1, "nonfinite": 1}
    m = ps.merge_probe([a, b])
    want = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [nan] * 4, [9, np.inf, 0, -1]], np.float32)
    assert np.array_equal(m["out4"].view(np.uint32), want.view(np.uint32))
    assert m["out4"].view(np.uint32)[2].tolist() == [0x7fc00000] * 4
    assert m["outcome"].tolist() == [0, 0, 1, 0]
    assert {k: m[k] for k in ("done", "served", "outside", "foreign", "nonfinite")} == {"done": 4, "served": 3, "outside": 1, "foreign": 0, "nonfinite": 1}
    assert ps.merge_probe([b, a])["out4"].tobytes() == m["out4"].tobytes()          # the ranks' order does not matter


def test_the_header_still_says_abi_8():
    text = open(os.path.join(ROOT, "include", "psamd.h")).read()
    assert int(re.search(r"#define PSAMD_ABI_VERSION (\d+)", text).group(1)) == 8 == ps.ABI_VERSION
    ps.build()
    assert ps.load().psamd_abi_version() == 8
