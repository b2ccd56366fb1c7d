"""The packing rule of the force pass's leftovers (csrc/pack_fit.hpp) without a GPU.

pack_fit_dump.cpp -- a stand-alone program, built with the address and undefined-behaviour sanitizers -- runs the serial
rule over the arrays below.  Checked: every cell with a leftover is in exactly one pack, no pack holds more than four cells
or 64 lanes, the count pass and the write pass agree, a pack's cells lie in one window of 64, and on the model of the
benchmark's cloud (4096 cells, Poisson(256) bodies, 57.9 % of them active) the rule needs at most 0.80 times the packs of
the next fit over runs of six cells it replaced (restated here; 0.76 measured)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pack_fit_model import as_rows, best_fit_packs

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "particlesystem_amd", "csrc")
WINDOW, LANES, GROUPS = 64, 64, 4
LENGTHS = (1, 27, 63, 64, 65, 125, 4096)


def model_leftovers(seed=2026, cells=4096):
    rng = np.random.default_rng(seed)
    return (rng.binomial(rng.poisson(256, cells), 0.579) & 63).astype(np.int64)


def arrays():
    rng = np.random.default_rng(7)
    out = {}
    for n in LENGTHS:
        out["zero_%d" % n] = np.zeros(n, np.int64)
        out["all63_%d" % n] = np.full(n, 63)
        out["all1_%d" % n] = np.ones(n, np.int64)
        out["all32_%d" % n] = np.full(n, 32)
        out["all33_%d" % n] = np.full(n, 33)
        out["32or33_%d" % n] = 32 + (np.arange(n) & 1)
        out["1and63_%d" % n] = np.where(np.arange(n) & 1, 63, 1)
        out["random_%d" % n] = rng.integers(0, 64, n)
        out["small_%d" % n] = rng.integers(0, 9, n)            # many to a pack: the four-cell limit binds
        out["sparse_%d" % n] = rng.integers(0, 64, n) * (rng.random(n) < 0.3)
    out["model"] = model_leftovers()
    return out


def next_fit_in_sixes(r):
    """the rule before: every thread of 1024 packs its own run of max(6, cells / 1024) cells by next fit, in cell order"""
    per = max(6, (len(r) + 1023) // 1024)
    packs = 0
    for p0 in range(0, len(r), per):
        used = ng = 0
        for v in r[p0:p0 + per]:
            if v == 0:
                continue
            if ng == 4 or used + v > 64:
                packs += 1
                used = ng = 0
            ng += 1
            used += v
        if ng:
            packs += 1
    return packs


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path_factory.mktemp("pack_fit") / "pack_fit_dump")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "pack_fit_dump.cpp"), "-o", exe], check=True)
    cases = arrays()
    text = "".join(" ".join(str(int(v)) for v in r) + "\n" for r in cases.values())
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True)
    assert out.stderr == ""
    lines = out.stdout.splitlines()
    got, at = {}, 0
    for name, r in cases.items():
        tag, n, counted, written = lines[at].split()
        assert tag == "N" and int(n) == len(r), (name, lines[at])
        packs = [tuple(int(x) for x in l.split()[1:]) for l in lines[at + 1:at + 1 + int(counted)]]
        assert all(l.startswith("P ") for l in lines[at + 1:at + 1 + int(counted)])
        got[name] = (r, int(counted), int(written), packs)
        at += 1 + int(counted)
    assert at == len(lines)
    return got


def test_every_leftover_in_exactly_one_pack_within_the_limits(packed):
    for name, (r, counted, written, packs) in packed.items():
        assert counted == written == len(packs), name
        seen = []
        for pk in packs:
            cells = [c for c in pk if c >= 0]
            assert 1 <= len(cells) <= GROUPS and pk[:len(cells)] == tuple(cells), (name, pk)    # filled from the front
            assert all(0 <= c < len(r) and r[c] > 0 for c in cells), (name, pk)
            assert sum(int(r[c]) for c in cells) <= LANES, (name, pk)
            assert len({c // WINDOW for c in cells}) == 1, (name, pk)
            seen += cells
        assert sorted(seen) == np.nonzero(r)[0].tolist(), name


def test_packs_are_numbered_window_by_window(packed):
    for name, (r, _, _, packs) in packed.items():
        wins = [pk[0] // WINDOW for pk in packs]
        assert wins == sorted(wins), name


def test_edge_arrays_give_the_counts_the_rule_implies(packed):
    for n in LENGTHS:
        full, rest = divmod(n, WINDOW)
        assert packed["zero_%d" % n][1] == 0
        assert packed["all63_%d" % n][1] == n and packed["all33_%d" % n][1] == n
        assert packed["all1_%d" % n][1] == full * (WINDOW // GROUPS) + (rest + GROUPS - 1) // GROUPS
        assert packed["all32_%d" % n][1] == full * (WINDOW // 2) + (rest + 1) // 2
        # 33s open a pack each (first: the larger), no 32 fits beside a 33, the 32s pair up
        n33 = [min(WINDOW, n - w) // 2 for w in range(0, n, WINDOW)]
        n32 = [min(WINDOW, n - w) - k for w, k in zip(range(0, n, WINDOW), n33)]
        assert packed["32or33_%d" % n][1] == sum(a + (b + 1) // 2 for a, b in zip(n33, n32))
        # a 63 takes exactly one 1
        ones = [(min(WINDOW, n - w) + 1) // 2 for w in range(0, n, WINDOW)]
        big = [min(WINDOW, n - w) // 2 for w in range(0, n, WINDOW)]
        assert packed["1and63_%d" % n][1] == sum(b + (max(0, a - b) + GROUPS - 1) // GROUPS for a, b in zip(ones, big))


def test_best_fit_places_by_decreasing_leftover(packed):
    """inside a pack the cells stand in the order they were placed: decreasing leftover, ties in cell order"""
    for name, (r, _, _, packs) in packed.items():
        for pk in packs:
            keys = [(-int(r[c]), c) for c in pk if c >= 0]
            assert keys == sorted(keys), (name, pk)


def test_packs_equal_the_python_restatement_pack_for_pack(packed):
    """best fit itself: first fit, another tie-break or another order of placement would give other packs"""
    for name, (r, _, _, packs) in packed.items():
        assert packs == as_rows(best_fit_packs(r)), name


def test_the_restatement_differs_from_first_fit_on_these_arrays(packed):
    """... and the arrays can tell: first fit decreasing packs some of them differently"""
    def first_fit(r):
        out = []
        for w0 in range(0, len(r), WINDOW):
            items = sorted((i for i in range(w0, min(len(r), w0 + WINDOW)) if r[i] > 0), key=lambda i: (-int(r[i]), i))
            mine = []
            for i in items:
                b = next((b for b in mine if len(b[1]) < GROUPS and b[0] + int(r[i]) <= LANES), None)
                if b is None:
                    b = [0, []]
                    mine.append(b)
                b[0] += int(r[i]); b[1].append(i)
            out += [b[1] for b in mine]
        return out
    assert any(as_rows(first_fit(r)) != packs for r, _, _, packs in packed.values())


def test_model_cloud_needs_four_fifths_of_the_packs_of_next_fit(packed):
    r, counted, _, _ = packed["model"]
    before = next_fit_in_sixes(r)
    print("packs: next fit in sixes %d, best fit decreasing over 64 cells %d, ratio %.3f" % (before, counted, counted / before))
    assert counted <= 0.80 * before
