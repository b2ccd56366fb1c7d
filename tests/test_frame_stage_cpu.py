"""The frame stage (csrc/frame_stage.hpp) against the flag machine it replaced, without a GPU.

frame_stage_dump.cpp -- a stand-alone program, built with the address and undefined-behaviour sanitizers -- prints
the whole table and the predicates.  This module holds the five flags the context had before (frame_reset,
grid_built, pairs_done, slab_stage, interior_done) with every call's test and assignments as step.hip, io.hip and
services.hip made them, and walks old and new side by side, breadth-first from a fresh context, over every call.

Where the two part ways, by design:
  * NEWLY_REFUSED: with world == 1 a call of one family inside a frame of the other.
  * the flags kept interior_done when fill / upload / inject / remove / snapshot_restore ended a slab frame between
    slab_pairs_interior and slab_pairs; the slab_pairs of the NEXT frame then ran the second pass alone.  The stage
    forgets the interior pass with the frame (STALE_INTERIOR is the one flag state that meets two stages)."""
import os
import shutil
import subprocess
from collections import deque

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "particlesystem_amd", "csrc")

PLAIN_CALLS = ("init_iframe", "build_grid", "calc_forces_pairs", "calc_forces_apply", "step")
SLAB_CALLS = ("slab_build", "slab_pairs_interior", "slab_pairs", "slab_apply", "slab_finish")
CALLS = PLAIN_CALLS + SLAB_CALLS + ("changed", "snapshot_restore")
PLAIN_FRAME = ("BUILT", "PAIRS")
SLAB_FRAME = ("SLAB_BUILT", "SLAB_INTERIOR", "SLAB_PAIRS", "SLAB_APPLIED")
STAGES = ("IDLE", "RESET") + PLAIN_FRAME + SLAB_FRAME

# (stage, call): what the flags let through and the table refuses
NEWLY_REFUSED = {(s, k) for s in SLAB_FRAME for k in ("init_iframe", "calc_forces_pairs", "step")} | \
                {("SLAB_PAIRS", "calc_forces_apply"), ("SLAB_APPLIED", "calc_forces_apply"),
                 ("BUILT", "slab_build"), ("PAIRS", "slab_build")}
#                 frame_reset, grid_built, pairs_done, slab_stage, interior_done
STALE_INTERIOR = (False, True, False, 1, True)


def old_call(state, call, world, have_interior):
    """the flag machine: None if the call was refused, else the flags it left"""
    R, B, Pd, S, I = state
    if call in PLAIN_CALLS and world > 1:
        return None                                     # slab_only
    if call == "init_iframe":
        return (True, False, False, S, I)
    if call == "build_grid":
        return (False, True, False, S, I) if R else None
    if call == "calc_forces_pairs":
        return (R, B, True, S, I) if B else None
    if call == "calc_forces_apply":
        return (R, False, False, S, I) if B and Pd else None        # finish_step
    if call == "step":
        return (False, False, False, S, I)              # frame_reset = false, built, pairs done; finish_step
    if call == "slab_build":
        return (False, True, False, 1, I)
    if call == "slab_pairs_interior":
        if S != 1:
            return None
        return state if (not have_interior or I) else (R, B, Pd, S, True)
    if call == "slab_pairs":
        return (R, B, True, 2, False) if S == 1 else None
    if call == "slab_apply":
        return (R, B, Pd, 3, I) if S == 2 else None
    if call == "slab_finish":
        return (R, False, False, 0, I) if S == 3 else None           # slab_stage = 0; finish_step
    if call == "changed":
        return (R, False, False, 0, I)                  # fill, upload, end_frame: frame_reset is left alone
    if call == "snapshot_restore":
        return (False, False, False, 0, I)              # end_frame; frame_reset = false
    raise AssertionError(call)


def old_predicates(state, world):
    R, B, Pd, S, I = state
    return B, Pd, (S == 2 if world > 1 else (B and S != 3))


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path_factory.mktemp("frame_stage") / "frame_stage_dump")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "frame_stage_dump.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    assert out.stderr == ""
    trans, pred, texts, mixed_text = {}, {}, {}, None
    for line in out.stdout.splitlines():
        tag, _, rest = line.partition(" ")
        if tag == "T":
            s, k, a, b = rest.split(" ")
            trans[(s, k)] = (a, b)                      # ("refuse", "mixed" | "order") or (stage left, stage left by a failed enqueue)
        elif tag == "P":
            s, *bits = rest.split(" ")
            pred[s] = tuple(b == "1" for b in bits)     # built, pairs_done, interior_done, field_window(1), field_window(2)
        elif tag == "R":
            k, _, text = rest.partition(" ")
            texts[k] = text
        elif tag == "M":
            mixed_text = rest
    assert set(trans) == {(s, k) for s in STAGES for k in CALLS} and set(pred) == set(STAGES)
    return trans, pred, texts, mixed_text


def new_call(trans, stage, call, world, have_interior):
    """step.hip's guard and the table; None if refused"""
    if call in PLAIN_CALLS and world > 1:
        return None
    to, _ = trans[(stage, call)]
    if to == "refuse":
        return None
    if call == "slab_pairs_interior" and not have_interior:
        return stage                                    # nothing to run: the call returns before it leaves
    return to


def walk(trans, pred, world, have_interior):
    start = ((False, False, False, 0, False), "IDLE")
    seen, todo = {start}, deque([start])
    met, refused = {}, set()
    while todo:
        old, new = todo.popleft()
        met.setdefault(old, set()).add(new)
        b, p, _, fw1, fw2 = pred[new]
        assert (b, p, fw2 if world > 1 else fw1) == old_predicates(old, world), (old, new)
        for call in CALLS:
            o, n = old_call(old, call, world, have_interior), new_call(trans, new, call, world, have_interior)
            if n is not None:
                assert o is not None, "the table accepts what the flags refused: %r %s %s" % (old, new, call)
            elif o is not None:
                assert (new, call) in NEWLY_REFUSED, "refused without being listed: %r %s %s" % (old, new, call)
                refused.add((new, call))
            if o is not None and n is not None and (o, n) not in seen:
                seen.add((o, n))
                todo.append((o, n))
    return met, refused


@pytest.mark.parametrize("have_interior", [False, True])
def test_world_one_differs_by_the_mixed_orders_alone(table, have_interior):
    trans, pred, _, _ = table
    met, refused = walk(trans, pred, 1, have_interior)
    # every member is met (the list holds nothing idle); a plan without an interior never stands at SLAB_INTERIOR
    assert refused == {(s, k) for s, k in NEWLY_REFUSED if have_interior or s != "SLAB_INTERIOR"}
    twice = {old: new for old, new in met.items() if len(new) > 1}
    assert twice == ({STALE_INTERIOR: {"SLAB_BUILT", "SLAB_INTERIOR"}} if have_interior else {})
    reached = set().union(*met.values())
    assert reached == set(STAGES) - (set() if have_interior else {"SLAB_INTERIOR"})


@pytest.mark.parametrize("have_interior", [False, True])
def test_world_two_differs_nowhere(table, have_interior):
    trans, pred, _, _ = table
    met, refused = walk(trans, pred, 2, have_interior)
    assert refused == set()
    twice = {old: new for old, new in met.items() if len(new) > 1}
    assert twice == ({STALE_INTERIOR: {"SLAB_BUILT", "SLAB_INTERIOR"}} if have_interior else {})
    assert set().union(*met.values()) == {"IDLE"} | set(SLAB_FRAME) - (set() if have_interior else {"SLAB_INTERIOR"})


def test_the_list_is_one_family_inside_the_others_frame(table):
    trans, _, _, _ = table
    for stage, call in NEWLY_REFUSED:
        assert (call in PLAIN_CALLS and stage in SLAB_FRAME) or (call in SLAB_CALLS and stage in PLAIN_FRAME), (stage, call)
    # ... and these are the refusals that carry the text naming both families, no others
    assert {sk for sk, (a, b) in trans.items() if a == "refuse" and b == "mixed"} == NEWLY_REFUSED


def test_refusal_texts_are_the_flag_machines(table):
    _, _, texts, mixed_text = table
    assert texts["build_grid"] == "build_grid needs init_iframe first"
    assert texts["calc_forces_pairs"] == "calc_forces needs build_grid first"
    assert texts["calc_forces_apply"] == "apply needs build_grid and the pair pass first"
    assert texts["slab_pairs_interior"] == "slab_pairs_interior belongs between slab_build and slab_pairs"
    assert texts["slab_pairs"] == "slab_pairs needs slab_build (and the halo exchange) first"
    assert texts["slab_apply"] == "slab_apply needs slab_pairs (and the force exchange) first"
    assert texts["slab_finish"] == "slab_finish needs slab_apply (and the transfer exchange) first"
    assert "init_iframe" in mixed_text and "slab_build" in mixed_text


def test_failed_enqueues_leave_what_the_flags_left(table):
    """a failed enqueue moved no flag, except that slab_pairs cleared interior_done before it looked at the status"""
    trans, _, _, _ = table
    for (stage, call), (to, failed) in trans.items():
        if to == "refuse":
            continue
        assert failed == ("SLAB_BUILT" if call == "slab_pairs" else stage), (stage, call, failed)
