"""The potential structs of include/psamd.h (psamd_potential_spec, psamd_potential_result) and their ctypes mirror
agree: a small C program compiled against the header prints sizeof / offsetof of every member, the mirror's layout must
match; the three entry points are declared, exported and bound, and refuse null arguments; the header still says ABI 8
(the feature adds entry points and structs, no layout moves)."""
import ctypes
import os
import re
import subprocess

import particlesystem_amd as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {"psamd_potential_spec": "Potential", "psamd_potential_result": "PotentialResult"}
ENTRY_POINTS = ("psamd_potential", "psamd_potential_result_get", "psamd_download_potential")


def c_layout(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "psamd.h"', "int main(void) {"]
    for cname, pyname in STRUCTS.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in getattr(ps, pyname)._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    # the entry points have the signatures the mirror binds
    lines.append("int (*f)(psamd_ctx *, const psamd_potential_spec *) = psamd_potential; (void)f;")
    lines.append("int (*g)(psamd_ctx *, psamd_potential_result *) = psamd_potential_result_get; (void)g;")
    lines.append("int (*h)(psamd_ctx *, float *, int64_t, psamd_potential_result *) = psamd_download_potential; (void)h;")
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


def test_potential_structs_match_the_ctypes_mirror(tmp_path):
    ps.build()
    got = c_layout(tmp_path)
    for cname, pyname in STRUCTS.items():
        py = getattr(ps, pyname)
        assert got[(cname, "sizeof")] == ctypes.sizeof(py), cname
        for field, _ in py._fields_:
            assert got[(cname, field)] == getattr(py, field).offset, (cname, field)
    assert got[("psamd_potential_result", "sizeof")] == 40 and got[("psamd_potential_spec", "sizeof")] == 32


def test_the_three_symbols_are_declared_exported_and_bound():
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
    assert lib.psamd_potential(None, None) == 1                      # PSAMD_ERR_INVALID_ARG
    assert lib.psamd_potential_result_get(None, None) == 1
    phi = (ctypes.c_float * 4)()
    out = ps.PotentialResult()
    assert lib.psamd_download_potential(None, ctypes.cast(phi, ctypes.c_void_p), 4, ctypes.byref(out)) == 1
    assert lib.psamd_download_potential(None, None, 0, None) == 1


def test_merge_potential_adds_counts_and_energy_and_takes_the_extrema():
    a = {"listed": 3, "nonfinite": 1, "potential": -2.0, "phi_min": -5.0, "phi_max": -1.0}
    b = {"listed": 4, "nonfinite": 0, "potential": -0.5, "phi_min": -3.0, "phi_max": -0.25}
    none = {"listed": 0, "nonfinite": 0, "potential": 0.0, "phi_min": float("inf"), "phi_max": float("-inf")}
    assert ps.merge_potential([a, b, none]) == {"listed": 7, "nonfinite": 1, "potential": -2.5, "phi_min": -5.0, "phi_max": -0.25}


def test_the_header_still_says_abi_8():
    text = open(os.path.join(ROOT, "include", "psamd.h")).read()
    assert int(re.search(r"#define PSAMD_ABI_VERSION (\d+)", text).group(1)) == 8 == ps.ABI_VERSION
    ps.build()
    assert ps.load().psamd_abi_version() == 8
