"""PSAMD_POTENTIAL_FAR | PSAMD_POTENTIAL_QUADRUPOLE and PSAMD_PROBE_FAR | PSAMD_PROBE_QUADRUPOLE on the device (include/psamd.h,
"energy", "the field at chosen points" and "quadrupoles on the pyramid").  What every method's field has is far_field_suite.py's,
taken from there under the names these nodes have had: phi and U against the numpy model (far_model.py; 1e-5 relative, the
standing bar of every far phi), the probes against the force records and against psamd_potential BIT FOR BIT, a confined cloud
(the cutoff context's bytes), the same bytes however the call is made, the captured graph, the statuses.  Here is what the
quadrupole method alone has: the quadrupole part alone, the limit in which every C is a zero (the pyramid context's bytes),
shuffled probes under a larger max_count.

Contexts hold max_particles_num=16384 (far_harness.py's GRID): 4^3 (one level), 6^3 (6, 3), 8^3 (8, 4), 10^3 (10, 5, 3: ragged) and
16^3 (16, 8, 4: levels of several blocks).

What was measured on an MI355X stands in the tests' docstrings."""
import numpy as np
import pytest
import torch

import far_field_suite as S
import far_model as F
from far_field_suite import EPS2, PYR, QUAD, scene, scene_of
from far_harness import DEV, bits, low_corner, make, open_frame, pos4_of, record, served

pytestmark = pytest.mark.gpu

shared = S.tests_of("quadrupole")
test_phi_and_U_follow_the_model = shared["phi_and_U_follow_the_model"]
test_probes_repeat_the_force_records_and_the_kids_phi_bit_for_bit = shared["probes_repeat_the_force_records_and_the_kids_phi_bit_for_bit"]
test_a_confined_cloud_is_the_cutoff_context_byte_for_byte = shared["confined_cloud_is_the_cutoff_context_byte_for_byte"]
test_the_same_bytes_before_and_after_the_pair_stage_and_nothing_else_moves = shared["the_same_bytes_before_and_after_the_pair_stage_and_nothing_else_moves"]
test_the_calls_are_captured_into_a_graph_and_replay_on_a_later_frame = shared["the_calls_are_captured_into_a_graph_and_replay_on_a_later_frame"]
test_the_status_table_cell_by_cell = shared["the_status_table_cell_by_cell"]


# ---- 1. the quadrupole part alone -----------------------------------------------------------------------------------------------

def test_the_quadrupole_part_alone():
    """8^3 cells, 16384 bodies (seed 52: chosen with the model on the CPU, where 60 % of the particles have a quadrupole part of at
    least 1e-4 of |phi|; median 1.25e-4).  phi of a quadrupole context under FAR | QUADRUPOLE minus phi of a pyramid context under
    FAR on the same cloud is the quadrupole chains' sum up to the fp32 rounding of the two records: about 1.2e-7 |phi|, which is
    1.2e-3 of a part of 1e-4 |phi|.  The bar of 1e-2 of the part leaves some 8 times that; a wrong coefficient or a swapped plane
    moves the part by tens of percent.  Measured on an MI355X: 59.7 % of the
    particles qualify; over them the difference is off by at most 9.3e-4 of the part (median 1.3e-4)"""
    G, n, seed = 8, 16384, 52
    a, b = scene(G, QUAD, 1.0, seed, n), scene(G, PYR, 1.0, seed, n)
    assert np.array_equal(a["order"], b["order"])
    xyz = a["c"]["xyz"]
    part = -F.quad_sum64(a["lists"], xyz, a["w_eff"], G, EPS2, xyz, a["cell"], a["moments"])      # (phi = -sum)
    got = a["phi"].astype(np.float64) - b["phi"].astype(np.float64)
    big = np.abs(part) >= 1e-4 * np.abs(a["phi"])
    rel = np.abs(got[big] - part[big]) / np.abs(part[big])
    print("the quadrupole part of phi alone, %d bodies on %d^3 cells: %.3f of the particles have a part of at least 1e-4 |phi|; over "
          "them, max deviation from the model's part %.3g of the part (median %.3g)" % (n, G, big.mean(), rel.max(), np.median(rel)))
    assert big.mean() >= 0.25
    assert rel.max() < 1e-2


# ---- 2. every C an exact zero: the pyramid context's bytes --------------------------------------------------------------------------

def test_one_adult_a_cell_is_the_pyramid_context_byte_for_byte():
    """4^3 cells with one adult each and 300 kids anywhere: every C is an exact zero and every quadrupole chain +0"""
    G = 4
    rng = np.random.default_rng(5)
    adults = np.array([low_corner(i1, i2, i3, G) for i3 in range(G) for i1 in range(G) for i2 in range(G)]) + rng.uniform(0.1, 4.9, (G ** 3, 3))
    xyz = np.concatenate([adults, rng.uniform(-9.9, 9.9, (300, 3))]).astype(np.float32)
    age = np.concatenate([np.full(G ** 3, 3.0), np.full(300, 0.5)]).astype(np.float32)
    w = rng.uniform(20.0, 100.0, len(xyz)).astype(np.float32)
    grid = pos4_of(rng.uniform(-9.9, 9.9, (500, 3)).astype(np.float32))
    got = []
    for flags in (QUAD, PYR):
        g = make(G, flags)
        g.fill_particles(xyz, age=age, w=w, fert_age=np.float32(1e6))
        open_frame(g)
        how = served(g, True)
        got.append((g.potential(phi=True, **how), g.probe(pos4_of(xyz), **how), g.probe(grid, **how)))
        g.calc_forces_pairs()
        if flags == QUAD:
            cen = g.download_level_quadrupoles(0)
            assert cen.shape == (G ** 3, 6) and not cen.view(np.uint32).any()      # (+0, every word)
            assert (g.download_level_moments(0)[:, 3] != 0).all()
        g.calc_forces_apply()
        g.close()
    (pa, oa, ga), (pb, ob, gb) = got
    assert pa["listed"] == len(xyz) and pa["potential"] < 0 and record(pa) == record(pb)
    assert np.array_equal(bits(pa["phi"]), bits(pb["phi"]))
    for x, y in ((oa, ob), (ga, gb)):
        assert x["served"] == y["served"] == len(x["out4"]) and np.array_equal(bits(x["out4"]), bits(y["out4"]))
    assert np.abs(oa["out4"].cpu().numpy()).min() > 0


# ---- 3. the same bytes however it is called ---------------------------------------------------------------------------------------

def test_two_calls_shuffled_probes_and_a_larger_max_count_give_the_same_bytes():
    G = 8
    s = scene_of("quadrupole", G)
    g = make(G, QUAD)
    g.fill_particles(**s["c"])
    open_frame(g)
    first = g.potential(phi=True, far=True, quadrupole=True)
    again = g.download_potential(far=True, quadrupole=True)
    m = 1500
    xyz = s["c"]["xyz"][:m]
    whole = g.probe(pos4_of(xyz), far=True, quadrupole=True)["out4"].cpu().numpy()
    g.calc_forces_pairs()                                                 # (the window stays open behind the pair stage)
    perm = np.random.default_rng(8).permutation(m)
    pad = np.concatenate([xyz[perm], np.full((700, 3), 1.0, np.float32)])
    count = torch.tensor([m], dtype=torch.int64, device=DEV)
    mixed = g.probe(pos4_of(pad), count=count, far=True, quadrupole=True)
    only_a = g.probe(pos4_of(xyz), phi=False, far=True, quadrupole=True)["out4"].cpu().numpy()
    only_p = g.probe(pos4_of(xyz), acc=False, far=True, quadrupole=True)["out4"].cpu().numpy()
    after = g.potential(phi=True, far=True, quadrupole=True)
    g.calc_forces_apply()
    g.close()
    for r in (again, after, s["res"]):
        assert np.array_equal(bits(r["phi"]), bits(first["phi"])) and record(r) == record(first)
    out = mixed["out4"].cpu().numpy()
    assert mixed["done"] == mixed["served"] == m and not out[m:].any()
    assert np.array_equal(bits(out[:m]), bits(whole[perm]))
    # where both are asked for, a body's front is formed once, in the acceleration's walk: the words of the walks of their own
    assert np.array_equal(bits(whole[:, :3]), bits(only_a[:, :3])) and np.array_equal(bits(whole[:, 3]), bits(only_p[:, 3]))
    assert np.abs(whole).min() > 0
