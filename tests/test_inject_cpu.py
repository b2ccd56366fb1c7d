"""The inject structs of include/psamd.h (psamd_inject_spec, psamd_inject_result) and their ctypes mirror agree: a
small C program compiled against the header prints sizeof / offsetof of every member, the mirror's layout must match;
the header's ABI version is the one the mirror is written for."""
import ctypes
import os
import re
import subprocess

import particlesystem_amd as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {"psamd_inject_spec": ps.Inject, "psamd_inject_result": ps.InjectResult}


def c_layout(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "psamd.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in py._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    # the entry points have the signatures the mirror binds
    lines.append("int (*f)(psamd_ctx *, const psamd_inject_spec *) = psamd_inject; (void)f;")
    lines.append("int (*g)(psamd_ctx *, psamd_inject_result *) = psamd_inject_result_get; (void)g;")
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


def test_inject_structs_match_the_ctypes_mirror(tmp_path):
    ps.build()
    got = c_layout(tmp_path)
    for cname, py in STRUCTS.items():
        assert got[(cname, "sizeof")] == ctypes.sizeof(py), cname
        for field, _ in py._fields_:
            assert got[(cname, field)] == getattr(py, field).offset, (cname, field)
    assert got[("psamd_inject_spec", "sizeof")] == 64 and got[("psamd_inject_result", "sizeof")] == 24


def test_abi_version_is_8_in_the_header_the_mirror_and_the_library():
    text = open(os.path.join(ROOT, "include", "psamd.h")).read()
    assert int(re.search(r"#define PSAMD_ABI_VERSION (\d+)", text).group(1)) == 8 == ps.ABI_VERSION
    ps.build()
    assert ps.load().psamd_abi_version() == 8


def test_the_mirror_binds_both_entry_points():
    names = [n for n, _, _ in ps.ABI]
    assert "psamd_inject" in names and "psamd_inject_result_get" in names
    lib = ps.load()
    assert lib.psamd_inject(None, None) == 1 and lib.psamd_inject_result_get(None, None) == 1     # PSAMD_ERR_INVALID_ARG
