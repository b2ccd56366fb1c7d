"""What context creation derives before it touches the device (csrc/context_params.hpp) without a GPU.

context_params_dump.cpp -- a stand-alone program, built with the address and undefined-behaviour sanitizers -- runs
derive_context_params over the configurations below and prints every field; context_params_model.py restates the rules from
the geometry (psamd_describe) and the ranks' plans (psamd_slab_plan_describe).  Every printed field of every configuration
must be the model's, floats by their bits; every refusal has a case with its status and a part of its text."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import particlesystem_amd as ps
from context_params_model import (ALL_PAIRS, EXPLOSIONS, FAR_MONOPOLE, FAR_PYRAMID, FAR_QUADRUPOLE, FAR_SLAB, INVALID_ARG, MSG_COUNT,
                                  UNSUPPORTED, largest_colliding_d2, model_of)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "particlesystem_amd", "csrc")
SMALL = dict(max_particles_num=4096)                                   # 16 cells per axis (the default chunks)
G8 = dict(max_particles_num=4096, chunk_factor=2, chunk_dim=4)
G10 = dict(max_particles_num=4096, chunk_factor=2, chunk_dim=5)        # no multiple of four
SINGLE = dict(collision_radius=0.0, chunk_factor=5, chunk_dim=3, max_particles_num=60000, cuts=[0, 2, 4, 6, 8, 10, 12, 15])
LEAN_LO = 2.0 ** -20                     # eps2^3 must exceed 2^-60
LEAN_HI = 2.0 ** 20 - 3.0 * 80.0 ** 2    # (3 (2 L)^2 + eps2)^3 must stay below 2^60; L = 8 cells of 5


def every_rank(world, **over):
    return [dict(over, world=world, rank=r) for r in range(world)]


def accepted():
    """name -> (overrides of the default configuration, PSAMD_ONE_PASS)"""
    c = {"world1": (SMALL, False), "one_pass": (SMALL, True), "one_pass_world2": (dict(SMALL, world=2, rank=1), True),
         "radius4_not_two_pass": (dict(SMALL, collision_radius=4.0), False),
         "drag_repulsion_seed": (dict(G8, drag=0.25, force_sign=-1.0, seed=2 ** 63 + 5, dt=0.01, life_steps=77.0), False),
         "grid40": (dict(chunk_factor=10, chunk_dim=4), False), "grid40_world4": (dict(chunk_factor=10, chunk_dim=4, world=4, rank=2), False),
         "eps2_low_end_out": (dict(G8, eps2=LEAN_LO), False), "eps2_low_end_in": (dict(G8, eps2=float(np.nextafter(LEAN_LO, 1.0))), False),
         "eps2_high_end_out": (dict(G8, eps2=LEAN_HI), False), "eps2_high_end_in": (dict(G8, eps2=float(np.nextafter(LEAN_HI, 0.0))), False),
         "allpairs_1": (dict(G10, flags=ALL_PAIRS), False)}
    for world in (2, 3, 4, 8):
        for o in every_rank(world, **SMALL):
            c["world%d_rank%d" % (world, o["rank"])] = (o, False)
    for name, world, cuts in (("cuts7", 2, [0, 7, 16]), ("cuts3", 2, [0, 3, 16]), ("cuts4", 4, [0, 4, 7, 11, 16])):
        for o in every_rank(world, cuts=cuts, **SMALL):
            c["%s_rank%d" % (name, o["rank"])] = (o, False)
    for o in every_rank(7, **SINGLE):
        c["single_layer_rank%d" % o["rank"]] = (o, False)
    for world in (4, 8):
        for o in every_rank(world, flags=EXPLOSIONS, **SMALL):
            c["explosions%d_rank%d" % (world, o["rank"])] = (o, False)
    for o in every_rank(3, flags=ALL_PAIRS, **G10):
        c["allpairs_3_rank%d" % o["rank"]] = (o, False)
    for name, flags in (("mono", FAR_MONOPOLE), ("pyramid", FAR_PYRAMID), ("quad", FAR_PYRAMID | FAR_QUADRUPOLE)):
        c["far_" + name] = (dict(SMALL, flags=flags), False)
        c["far_%s_slab_world1" % name] = (dict(SMALL, flags=flags | FAR_SLAB), False)
        for o in every_rank(2, flags=flags | FAR_SLAB, **SMALL):
            c["far_%s_slab_rank%d" % (name, o["rank"])] = (o, False)
    c["far_pyramid_grid10_slab3"] = (dict(G10, flags=FAR_PYRAMID | FAR_SLAB | EXPLOSIONS, world=3, rank=1), False)
    for name, caps in (("halo_cap_3", dict(halo_cap_cell=3)), ("halo_cap_too_big", dict(halo_cap_cell=1000)), ("xfer_cap_100", dict(xfer_cap=100)),
                       ("xfer_max_below_cap", dict(xfer_cap=100, xfer_cap_max=50)), ("xfer_max_5000", dict(xfer_cap_max=5000)),
                       ("xfer_all", dict(xfer_cap=64, xfer_cap_max=9000, halo_cap_cell=2))):
        c[name] = (dict(SMALL, world=3, rank=1, cuts=[0, 4, 7, 16], **caps), False)
    return c


def refused():
    """name -> (overrides, status, a part of the refusal's text).  The one refusal without a case is the rank loop's "no slab
    partition for this grid and world size" (without the own plan's "every rank needs"): see test_plans_stand_or_fall_together."""
    mono, pyr = "far monopoles", "the pyramid of monopoles"
    return {
        "rank_beyond_world": (dict(SMALL, world=2, rank=2), INVALID_ARG, "rank/world"),
        "world_0": (dict(SMALL, world=0), INVALID_ARG, "rank/world"),
        "world_65": (dict(SMALL, world=65), INVALID_ARG, "rank/world"),
        "no_plan": (dict(G8, world=8, rank=3), UNSUPPORTED, "every rank needs >= 2 cell layers"),
        "drag": (dict(SMALL, drag=-0.5), INVALID_ARG, "drag must be >= 0"),
        "slab_alone": (dict(SMALL, flags=FAR_SLAB), INVALID_ARG, "PSAMD_FLAG_FAR_SLAB is a modifier of"),
        "key_64_bits": (dict(chunk_factor=40, chunk_dim=3, x_factor=20), UNSUPPORTED, "queue-op key does not fit 64 bits"),
        "allpairs_not_lean": (dict(SMALL, flags=ALL_PAIRS, eps2=1e-8), UNSUPPORTED, "all-pairs forces are built for the lean pair arithmetic"),
        "allpairs_not_two_pass": (dict(SMALL, flags=ALL_PAIRS, collision_radius=4.0), UNSUPPORTED, "all-pairs forces need the two-pass pair stage"),
        "quadrupole_alone": (dict(SMALL, flags=FAR_QUADRUPOLE), INVALID_ARG, "quadrupoles (PSAMD_FLAG_FAR_QUADRUPOLE) belong to the pyramid"),
        "quadrupole_flat": (dict(SMALL, flags=FAR_QUADRUPOLE | FAR_MONOPOLE), INVALID_ARG, "set PSAMD_FLAG_FAR_PYRAMID too"),
        "mono_and_allpairs": (dict(SMALL, flags=FAR_MONOPOLE | ALL_PAIRS), INVALID_ARG, "far monopoles and all-pairs forces are two force models"),
        "pyramid_and_allpairs": (dict(SMALL, flags=FAR_PYRAMID | ALL_PAIRS), INVALID_ARG, "are three force models: choose one"),
        "mono_world2": (dict(SMALL, flags=FAR_MONOPOLE, world=2), UNSUPPORTED, mono + " are served on one context only (world == 1)"),
        "pyramid_world2": (dict(SMALL, flags=FAR_PYRAMID, world=2, rank=1), UNSUPPORTED, pyr + " is served on one context only"),
        "mono_not_lean": (dict(SMALL, flags=FAR_MONOPOLE, eps2=1e-8), UNSUPPORTED, mono + " are built for the lean pair arithmetic only"),
        "pyramid_not_lean": (dict(SMALL, flags=FAR_PYRAMID | FAR_SLAB, eps2=1e-8, world=2), UNSUPPORTED, pyr + " is built for the lean"),
        "mono_not_two_pass": (dict(SMALL, flags=FAR_MONOPOLE, collision_radius=4.0), UNSUPPORTED, mono + " need the two-pass pair stage"),
        "pyramid_one_pass": (dict(SMALL, flags=FAR_PYRAMID), UNSUPPORTED, pyr + " needs the two-pass pair stage"),
        "mono_and_pyramid": (dict(SMALL, flags=FAR_MONOPOLE | FAR_PYRAMID), INVALID_ARG, "the pyramid of monopoles, far monopoles and all-pairs forces are three"),
    }


ONE_PASS_REFUSALS = ("pyramid_one_pass",)


def line_of(cfg, one_pass):
    cuts = list(cfg.cuts)
    return " ".join([str(v) for v in (cfg.max_particles_num, cfg.x_factor, cfg.chunk_factor, cfg.chunk_dim)]
                    + [repr(float(v)) for v in (cfg.cell_size, cfg.eps2, cfg.collision_radius, cfg.particle_weight, cfg.dt, cfg.max_v,
                                                cfg.explosion_speed, cfg.life_steps)]
                    + [str(v) for v in (cfg.flags, cfg.seed, cfg.rank, cfg.world, cfg.halo_cap_cell, cfg.xfer_cap, cfg.xfer_cap_max)]
                    + [repr(float(cfg.drag)), repr(float(cfg.force_sign)), str(int(one_pass)), str(len(cuts))] + [str(v) for v in cuts]) + "\n"


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """name -> (configuration, PSAMD_ONE_PASS, status, why, {field: [numbers]}) for the accepted and the refused ones"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the stand-alone program"
    exe = str(tmp_path_factory.mktemp("context_params") / "context_params_dump")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "context_params_dump.cpp"), "-o", exe], check=True)
    cases = {k: (ps.default_config(**o), one_pass) for k, (o, one_pass) in accepted().items()}
    cases.update({k: (ps.default_config(**o), k in ONE_PASS_REFUSALS) for k, (o, _, _) in refused().items()})
    out = subprocess.run([exe], input="".join(line_of(cfg, op) for cfg, op in cases.values()), check=True, capture_output=True, text=True)
    assert out.stderr == ""
    blocks = out.stdout.split("end\n")
    assert blocks[-1] == "" and len(blocks) == len(cases) + 1
    got = {}
    for (name, (cfg, one_pass)), block in zip(cases.items(), blocks):
        lines = block.splitlines()
        assert lines[0].startswith("status ") and lines[1].startswith("why"), (name, lines[:2])
        fields = {}
        for l in lines[2:]:
            key, *vals = l.split()
            assert key not in fields, (name, key)
            fields[key] = [int(v, 0) for v in vals]
        got[name] = (cfg, one_pass, int(lines[0].split()[1]), lines[1][4:], fields)
    return got


def test_every_field_of_every_configuration_is_the_models(dumped):
    for name in accepted():
        cfg, one_pass, status, why, fields = dumped[name]
        assert status == 0 and why == "", (name, status, why)
        model = model_of(cfg, one_pass)
        assert isinstance(model, dict), (name, model)
        assert sorted(fields) == sorted(model), (name, sorted(set(fields) ^ set(model)))
        for key, want in model.items():
            assert fields[key] == [int(v) for v in want], (name, key, fields[key], want)


def test_every_refusal_has_its_status_and_text(dumped):
    for name, (_, want, text) in refused().items():
        cfg, one_pass, status, why, fields = dumped[name]
        assert status == want and text in why and not fields, (name, status, why)
        assert model_of(cfg, one_pass) == want, name


def test_the_cases_reach_what_they_are_there_for(dumped):
    f = {name: dumped[name][4] for name in accepted()}
    assert f["single_layer_rank2"]["P.xfer2_cap"] == [1024] and f["single_layer_rank3"]["P.reg_layers"][0] == 1
    assert f["single_layer_rank2"]["msg.15"][0] > 0 and f["world4_rank1"]["P.xfer2_cap"] == [0]
    assert f["explosions4_rank0"]["P.far_cap"] == [16] and f["explosions4_rank0"]["msg.19"][0] == 4 * f["explosions4_rank0"]["msg.18"][0] > 0
    assert f["world4_rank0"]["P.far_cap"] == [0] and f["world3_rank0"]["msg.18"] == [0, 0]
    # a cut inside a group lends layers (the balanced cut at 8, the cut at 4); the cuts at 7 and 3 are group-aligned: a halo above instead
    assert f["world2_rank1"]["P.reg_layers"][2] == 1 and f["world2_rank0"]["msg.5"][0] > 0 and f["cuts4_rank1"]["msg.4"][0] > 0
    assert f["cuts7_rank1"]["P.reg_layers"] == [9, 1, 0, 0] and f["cuts7_rank0"]["P.reg_layers"] == [7, 0, 0, 1] and f["cuts3_rank0"]["msg.3"][0] > 0
    assert f["allpairs_3_rank1"]["msg.13"][1] == f["allpairs_3_rank1"]["msg.13"][0] + 256
    assert f["far_quad_slab_rank1"]["P.allg_block"] == [(64 + 10 * 8 * f["far_quad_slab_rank1"]["P.allg_cells"][0]) // 4]
    assert len(f["far_quad_slab_rank1"]["far_plan"]) == 4 and f["far_quad"]["lev.n"] == [3] and f["far_mono"]["lev.n"] == [1]
    assert (f["eps2_low_end_out"]["P.lean_math"], f["eps2_low_end_in"]["P.lean_math"]) == ([0], [1])
    assert (f["eps2_high_end_out"]["P.lean_math"], f["eps2_high_end_in"]["P.lean_math"]) == ([0], [1])
    assert f["radius4_not_two_pass"]["P.two_pass"] == [0] and f["one_pass"]["P.two_pass"] == [0] and f["world1"]["P.two_pass"] == [1]
    assert f["grid40"]["P.key_bits"] > f["world1"]["P.key_bits"] and f["grid40"]["P.key_bits"][0] <= 63
    assert f["halo_cap_3"]["P.halo_cap_cell"] == [3] and f["halo_cap_too_big"]["P.halo_cap_cell"] == f["halo_cap_too_big"]["P.max_per_cell"]
    assert f["xfer_max_below_cap"]["P.xfer_cap_max"] == [100] and f["xfer_max_5000"]["P.xfer_cap_max"] == [5000]
    assert any(v["have_interior"] == [1] for v in f.values()) and f["one_pass_world2"]["have_interior"] == [0]


def cells(lo, hi):
    return [c for a, b in zip(lo, hi) for c in range(a, b)]


def test_interior_and_rest_partition_the_computed_cells(dumped):
    split = 0
    for name in accepted():
        f = dumped[name][4]
        comp, inner, rest = cells(f["P.comp_lo"], f["P.comp_hi"]), cells(f["int_lo"], f["int_hi"]), cells(f["rest_lo"], f["rest_hi"])
        assert len(set(comp)) == len(comp), name
        if f["have_interior"] == [1]:
            split += 1
            assert inner and rest and not set(inner) & set(rest) and len(inner) + len(rest) == len(comp), name
            assert sorted(inner + rest) == sorted(comp), name
        else:
            assert inner == rest == comp, name
    assert split >= 10


def test_largest_colliding_d2_is_the_edge():
    """the model's statement of coll_d2_max, on its own: the square root of t, as a double, is within the radius and that of the
    next float is not"""
    for radius in (0.4, 4.0, 0.0, 1e-30, 1.0, 0.1 + 2.0 ** -30, 3.0e18):
        t = largest_colliding_d2(radius)
        assert float(np.sqrt(t)) <= radius < float(np.sqrt(np.nextafter(t, np.float32(np.inf)))), radius
    assert largest_colliding_d2(-1.0) == np.float32(-1.0)


def test_plans_stand_or_fall_together():
    """Why one refusal has no case: derive_context_params refuses a configuration whose own plan stands while another rank's
    falls, and on 16 layers no list of cuts of two layers or more makes such a world."""
    for world in (2, 3, 4):
        for inner in itertools.combinations(range(2, 15), world - 1):
            cuts = [0] + list(inner) + [16]
            if min(b - a for a, b in zip(cuts, cuts[1:])) < 2:
                continue
            ok = set()
            for r in range(world):
                try:
                    ps.slab_plan(ps.default_config(rank=r, world=world, cuts=cuts))
                    ok.add(True)
                except ps.PsamdError:
                    ok.add(False)
            assert len(ok) == 1, cuts
    assert MSG_COUNT == 20
