"""The export structs of include/psamd.h (psamd_live_stats, psamd_export) and their ctypes mirror agree: a small C
program compiled against the header prints sizeof / offsetof of every member, the mirror's layout must match."""
import ctypes
import os
import re
import subprocess

import particlesystem_amd as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {"psamd_live_stats": ps.LiveStats, "psamd_export": ps.Export}


def c_layout(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "psamd.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in py._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-x", "c++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {tuple(l.split()[:2]): int(l.split()[2]) for l in out.splitlines()}


def test_export_structs_match_the_ctypes_mirror(tmp_path):
    got = c_layout(tmp_path)
    for cname, py in STRUCTS.items():
        assert got[(cname, "sizeof")] == ctypes.sizeof(py), cname
        for field, _ in py._fields_:
            assert got[(cname, field)] == getattr(py, field).offset, (cname, field)
    assert got[("psamd_live_stats", "sizeof")] == 152 and got[("psamd_export", "sizeof")] == 72


def test_export_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "psamd.h")).read()
    for name in ("POS", "VEL", "ACC", "ID", "CELL", "ALL"):
        m = re.search(r"#define PSAMD_EXPORT_%s\s+(0x[0-9a-f]+)u" % name, text)
        assert m, name
        assert int(m.group(1), 16) == getattr(ps, "EXPORT_" + name), name


def test_merge_live_stats_adds_counts_and_sums_and_takes_the_extrema():
    a = {"live": 3, "nonfinite": 1, "mass": 1.5, "momentum": [1.0, 2.0, 3.0], "kinetic": 0.25, "mass_moment": [0.0, 1.0, -1.0],
         "lo": [-1.0, -2.0, 0.0], "hi": [1.0, 0.5, 4.0], "age_min": 0.5, "age_max": 2.0, "age_sum": 3.0}
    b = {"live": 2, "nonfinite": 0, "mass": 0.5, "momentum": [-1.0, 0.0, 1.0], "kinetic": 0.75, "mass_moment": [2.0, 2.0, 2.0],
         "lo": [-3.0, 0.0, 1.0], "hi": [0.0, 9.0, 2.0], "age_min": 0.25, "age_max": 1.0, "age_sum": 1.0}
    empty = {"live": 0, "nonfinite": 0, "mass": 0.0, "momentum": [0.0] * 3, "kinetic": 0.0, "mass_moment": [0.0] * 3,
             "lo": [float("inf")] * 3, "hi": [float("-inf")] * 3, "age_min": float("inf"), "age_max": float("-inf"), "age_sum": 0.0}
    m = ps.merge_live_stats([a, empty, b])
    assert m["live"] == 5 and m["nonfinite"] == 1 and m["mass"] == 2.0 and m["kinetic"] == 1.0 and m["age_sum"] == 4.0
    assert list(m["momentum"]) == [0.0, 2.0, 4.0] and list(m["mass_moment"]) == [2.0, 3.0, 1.0]
    assert list(m["lo"]) == [-3.0, -2.0, 0.0] and list(m["hi"]) == [1.0, 9.0, 4.0]
    assert m["age_min"] == 0.25 and m["age_max"] == 2.0


def test_driver_accepts_the_frame_options_on_the_host_only_path():
    """--frames / --frame-every parse without a GPU (--describe stops before the device is touched)"""
    from particlesystem_amd import _build as psbuild
    exe = psbuild.build_driver()
    out = subprocess.run([exe, "--describe", "--frames", "/nonexistent", "--frame-every", "5"], check=True,
                         capture_output=True, text=True).stdout
    assert out.startswith("grid ")
