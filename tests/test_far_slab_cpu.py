"""The far field on slabs (PSAMD_FLAG_FAR_SLAB) without a GPU: the flag in the header and its Python mirror, the ring host's
--far option through the hooks that need no GPU, and the HIP-free host code -- the option parser, the slab plans, the size of the
all-gathered block of cell sums -- built as a stand-alone program with the host sanitizers and run once."""
import os
import re
import subprocess

import pytest

import particlesystem_amd as ps
from far_harness import GRID

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_flag_in_the_header_and_its_mirror():
    text = open(os.path.join(ROOT, "include", "psamd.h")).read()
    m = re.search(r"#define\s+PSAMD_FLAG_FAR_SLAB\s+(0x[0-9a-fA-F]+)u", text)
    assert m and int(m.group(1), 16) == 0x80 == ps.FLAG_FAR_SLAB
    assert re.search(r"#define\s+PSAMD_ABI_VERSION\s+8\b", text) and ps.ABI_VERSION == 8
    others = [ps.FLAG_EXPLOSIONS, ps.FLAG_FAST_MATH, ps.FLAG_ALL_PAIRS, ps.FLAG_EULER, ps.FLAG_FAR_MONOPOLE, ps.FLAG_FAR_PYRAMID, ps.FLAG_FAR_QUADRUPOLE]
    assert all(ps.FLAG_FAR_SLAB & f == 0 for f in others)


def ring(*args):
    exe = ps._build.build_ring()
    return subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=30)


@pytest.mark.parametrize("far", ["flat", "pyramid", "quadrupole"])
def test_far_option_parses(far):
    p = ring("--routes", "--world", "3", "--rank", "1", "--far", far)
    assert p.returncode == 0 and p.stdout.startswith("send "), p.stdout       # (the routes do not change: the slot is all-gathered)
    assert p.stdout == ring("--routes", "--world", "3", "--rank", "1").stdout


def test_far_option_refusals():
    p = ring("--routes", "--world", "2", "--far", "pyramid", "--all-pairs")
    assert p.returncode == 2 and "--far and --all-pairs" in p.stdout
    for bad in (["--far", "octupole"], ["--far"]):
        p = ring("--routes", "--world", "2", *bad)
        assert p.returncode == 2 and "flat, pyramid or quadrupole" in p.stdout
    # ... and "--far" as another option's value is that option's value, not a far model left out
    assert ring("--routes", "--world", "2", "--id-file", "--far").returncode == 0


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("far_slab_host") / "far_slab_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "far_slab_host", "main.cpp"), "-o", exe], check=True)
    return exe


def test_host_code_under_the_sanitizers(host_program):
    """16^3 cells on four ranks with the uneven cuts, quadrupoles: the plans' state layers are 3, 4, 4, 5, every block has room for
    the five; the program's numbers are the library's own plan (psamd_slab_plan_describe)."""
    G, world, cuts = 16, 4, (0, 3, 7, 11, 16)
    p = subprocess.run([host_program, "--routes", "--world", str(world), "--far", "quadrupole", "--cuts", ",".join(map(str, cuts))],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 0 and p.stderr == "", (p.stdout, p.stderr)
    rows = [[int(t) for t in ln.split()] for ln in p.stdout.splitlines()]
    plans = [ps.slab_plan(ps.default_config(rank=r, world=world, cuts=cuts, **GRID[G])) for r in range(world)]
    cells = [(q.state_hi - q.state_lo) * G * G for q in plans]
    assert rows[0] == [3, 10, max(cells), 64 + 10 * max(cells) * 8]
    assert rows[1:] == [[q.state_lo * G * G, n] for q, n in zip(plans, cells)]
    assert len(set(cells)) > 1 and sum(cells) == G ** 3


def test_host_code_refuses_what_the_parser_refuses(host_program):
    p = subprocess.run([host_program, "--routes", "--world", "2", "--far", "pyramid", "--all-pairs"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 2 and "two force models" in p.stderr
    p = subprocess.run([host_program, "--routes", "--world", "9", "--far", "flat"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 1 and "no slab partition" in p.stderr      # (16 layers do not make nine slabs of two)
