"""PSAMD_POTENTIAL_FAR and PSAMD_PROBE_FAR on the device (include/psamd.h, "energy" and "the field at chosen points", far-
monopole contexts).  What every method's field has is far_field_suite.py's, taken from there under the names these nodes have
had: phi and U against the numpy model (far_model.py; 1e-5 relative, psamd_potential's bar), a confined cloud (the cutoff
context's bytes), the probe's acceleration against the force records BIT FOR BIT, the same bytes however the call is made, the
captured graph, the statuses.  Here is what the flat and the pyramid method alone have: G = 4 is the flat context's bytes, one adult
per cell against an all-pairs context, a list of two slices, fast math, the probe's phi on a grid with points outside the box.

Contexts hold max_particles_num=16384 (far_harness.py's GRID): 4^3 (one level), 8^3 (8, 4), 10^3 (10, 5, 3: ragged)
and 16^3 (16, 8, 4: levels of several blocks)."""
import numpy as np
import pytest

import far_field_suite as S
import far_model as F
import particlesystem_amd as ps
from far_field_suite import EPS2, REL, scene_of
from far_harness import bits, body_cloud, by_fill, fill_lists, low_corner, make, open_frame, pos4_of, record

pytestmark = pytest.mark.gpu

PYR, MONO = ps.FLAG_FAR_PYRAMID, ps.FLAG_FAR_MONOPOLE
FLAG = {"flat": MONO, "pyramid": PYR}
BOTH = pytest.mark.parametrize("method", ["flat", "pyramid"])

shared = S.tests_of("flat", "pyramid")
test_phi_and_U_follow_the_model = shared["phi_and_U_follow_the_model"]
test_confined_cloud_is_the_cutoff_result_byte_for_byte = shared["confined_cloud_is_the_cutoff_context_byte_for_byte"]
test_an_acc_probe_on_a_served_adult_is_its_force_record_bit_for_bit = shared["probes_repeat_the_force_records_and_the_kids_phi_bit_for_bit"]
test_the_same_bytes_before_and_after_the_pair_stage_and_nothing_else_moves = shared["the_same_bytes_before_and_after_the_pair_stage_and_nothing_else_moves"]
test_the_far_call_is_captured_into_a_graph_and_replays_on_a_later_frame = shared["the_calls_are_captured_into_a_graph_and_replay_on_a_later_frame"]
test_refusals_and_arguments = shared["the_status_table_cell_by_cell"]


# ---- 1. one level ------------------------------------------------------------------------------------------------------------

def test_one_level_is_the_flat_context_byte_for_byte():
    c = body_cloud(2048, 81, 4)
    got = []
    for flag in (PYR, MONO):
        g = make(4, flag)
        g.fill_particles(**c)
        open_frame(g)
        got.append(g.potential(phi=True, far=True))
        near = g.probe(pos4_of(c["xyz"]), far=True)
        got.append(near["out4"])
        g.calc_forces()
        g.close()
    assert got[0]["listed"] == 2048 and np.array_equal(bits(got[0]["phi"]), bits(got[2]["phi"])) and record(got[0]) == record(got[2])
    assert np.array_equal(bits(got[1]), bits(got[3]))
    s = np.abs(got[0]["phi"].cpu().numpy())
    assert s.min() > 0


# ---- 2. one adult per cell ------------------------------------------------------------------------------------------------

def test_one_adult_per_cell_is_the_all_pairs_phi():
    """at most one adult (and some kids) a cell: the cells' monopoles ARE the adults, every far body of the flat method is
    exact.  (Not so for the pyramid, whose coarser levels merge adults: it has no such limit.)"""
    G, flag = 8, MONO
    rng = np.random.default_rng(91)
    cells = rng.choice(G ** 3, 300, replace=False)
    i3, rem = np.divmod(cells, G * G)
    i1, i2 = np.divmod(rem, G)
    xyz = np.array([low_corner(a, b, c, G) for a, b, c in zip(i1, i2, i3)]) + rng.uniform(0.1, 4.9, (300, 3))
    kids = xyz[:40] + rng.uniform(-0.05, 0.05, (40, 3))
    xyz = np.concatenate([xyz, kids]).astype(np.float32)
    age = np.concatenate([np.full(300, 3.0), np.full(40, 0.5)]).astype(np.float32)
    w = rng.uniform(20.0, 100.0, 340).astype(np.float32)
    got = []
    for flags in (flag, ps.FLAG_ALL_PAIRS):
        g = make(G, flags)
        g.fill_particles(xyz, age=age, w=w, fert_age=np.float32(1e6))
        open_frame(g)
        got.append(g.download_potential(far=flags == flag))
        g.calc_forces()
        g.close()
    a, b = got[0]["phi"].astype(np.float64), got[1]["phi"].astype(np.float64)
    rel = np.abs(a - b) / np.abs(b)
    print("one adult a cell, flags %#x: far phi against the all-pairs context's, max %.3g; U %.3g"
          % (flag, rel.max(), abs(got[0]["potential"] - got[1]["potential"]) / abs(got[1]["potential"])))
    assert got[0]["listed"] == got[1]["listed"] == 340
    assert rel.max() < REL and abs(got[0]["potential"] - got[1]["potential"]) < REL * abs(got[1]["potential"])


# ---- 3. a list of two slices ------------------------------------------------------------------------------------------------

@BOTH
def test_both_slices_of_a_long_list_carry_the_far_part(method):
    G, flag = 8, FLAG[method]
    g = make(G, flag)
    many = g.sizes.max_per_cell                                           # a full list: 64 lanes and a ragged second slice
    assert 64 < many < 128
    c = body_cloud(3000, 95, G)
    rng = np.random.default_rng(96)
    crowd = (low_corner(4, 2, 3, G) + rng.uniform(0.05, 4.95, (many, 3))).astype(np.float32)
    full = (3 * G + 4) * G + 2
    keep = F.cells_of(c["xyz"], G) != full
    xyz = np.concatenate([c["xyz"][keep], crowd])
    age = np.concatenate([c["age"][keep], np.full(many, 3.0, np.float32)])
    w = np.concatenate([c["w"][keep], np.full(many, 60.0, np.float32)])
    ids = g.fill_particles(xyz, age=age, w=w, fert_age=np.float32(1e6))
    open_frame(g)
    res = g.potential(phi=True, far=True)
    ex = g.export_live(ps.EXPORT_ID | ps.EXPORT_POS)
    lists, _ = fill_lists(g, ids)
    g.calc_forces()
    kills = g.counters["cell_overflow_kills"]
    g.close()
    assert len(lists[full]) == many and kills == 0
    assert np.array_equal(ex["id"].cpu().numpy(), np.sort(ids)) and len(res["phi"]) == len(ids)
    where = np.full(ids.max() + 1, -1)
    where[ids] = np.arange(len(ids))
    assert np.array_equal(ex["pos4"].cpu().numpy()[:, :3], xyz[where[ex["id"].cpu().numpy()]])      # entry for entry with the export
    phi = by_fill(ids, res["phi"])
    w_eff = np.where(age < 1.5, np.float32(0), w).astype(np.float32)
    crowd_idx = lists[full]
    cell = np.full(many, full)
    want = F.phi64(lists, xyz, w_eff, G, EPS2, xyz[crowd_idx], cell, crowd_idx, method)
    near = F.phi64(lists, xyz, w_eff, G, EPS2, xyz[crowd_idx], cell, crowd_idx, method, far=False)
    rel = np.abs(phi[crowd_idx] - want) / np.abs(want)
    print("a list of %d, flags %#x: max relative deviation %.3g (first slice %.3g, second %.3g); far part %.3g of phi"
          % (many, flag, rel.max(), rel[:64].max(), rel[64:].max(), np.median(1 - near / want)))
    assert rel.max() < REL and np.median(1 - near / want) > 100 * REL    # (a slice without its far part would miss by that much)


# ---- 4. fast math -----------------------------------------------------------------------------------------------------------

@BOTH
def test_fast_math_probes_give_the_same_bytes_twice_and_follow_the_model(method):
    G, flag = 8, FLAG[method]
    s = scene_of(method, G)
    adults = np.nonzero(~s["kid"])[0][:2000]
    outs = []
    for _ in range(2):
        g = make(G, flag | ps.FLAG_FAST_MATH)
        g.fill_particles(**s["c"])
        open_frame(g)
        outs.append(g.probe(pos4_of(s["c"]["xyz"][adults]), far=True)["out4"].cpu().numpy())
        g.calc_forces()
        g.close()
    assert outs[0].tobytes() == outs[1].tobytes()
    want = F.accel64(s["lists"], s["c"]["xyz"], s["w_eff"], G, EPS2, s["c"]["xyz"][adults], s["cell"][adults], method, s["moments"])
    rel = F.rel_dev(outs[0][:, :3].astype(np.float64), want)
    print("fast-math far probes, flags %#x: max relative deviation of a from the model %.3g" % (flag, rel.max()))
    assert rel.max() < REL


# ---- 5. the probe's phi ---------------------------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("G", [8, 16])
def test_probe_phi(G, method):
    flag = FLAG[method]
    s = scene_of(method, G)
    c, n = s["c"], len(s["ids"])
    g = make(G, flag)
    g.fill_particles(**c)
    open_frame(g)
    on = g.probe(pos4_of(c["xyz"]), acc=False, far=True)["out4"].cpu().numpy()[:, 3]
    # a regular grid of points, two of them outside the box and one not a number
    k = np.arange(12)
    half = G * 2.5
    grid = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3) * (2 * half / 12) - half + 0.37
    grid = np.concatenate([grid, [[half + 1.0, 0, 0], [0, -half - 3.0, 0], [np.nan, 0, 0]]]).astype(np.float32)
    res = g.probe(pos4_of(grid), far=True, outcome=True)
    g.calc_forces()
    g.close()
    kid = s["kid"]
    assert np.array_equal(bits(on[kid]), bits(s["phi"][kid]))             # a kid's true position: its far phi, bit for bit
    own = -(s["w_eff"][~kid].astype(np.float64)) / np.sqrt(np.float64(np.float32(EPS2)))
    rel = np.abs(on[~kid] - (s["phi"][~kid].astype(np.float64) + own)) / np.abs(on[~kid])
    out4, code = res["out4"].cpu().numpy(), res["outcome"].cpu().numpy()
    assert code[-3:].tolist() == [ps.PROBE_OUTSIDE] * 3 and (bits(out4[-3:]) == 0x7fc00000).all() and (code[:-3] == ps.PROBE_SERVED).all()
    assert res["served"] == 12 ** 3 and res["outside"] == 3 and res["nonfinite"] == 0
    cell = F.cells_of(grid[:-3], G)
    minus = np.full(len(cell), -1)
    want = F.phi64(s["lists"], c["xyz"], s["w_eff"], G, EPS2, grid[:-3], cell, minus, method, s["moments"])
    wacc = F.accel64(s["lists"], c["xyz"], s["w_eff"], G, EPS2, grid[:-3], cell, method, s["moments"])
    rphi = np.abs(out4[:-3, 3] - want) / np.abs(want)
    racc = F.rel_dev(out4[:-3, :3].astype(np.float64), wacc)
    print("far probes on %d^3 cells, flags %#x: on adults, phi + own term to %.3g; on a grid phi to %.3g, a to %.3g"
          % (G, flag, rel.max(), rphi.max(), racc.max()))
    assert rel.max() < 4 * 2.0 ** -24                                     # two roundings to fp32 and the sum's: "to rounding"
    assert rphi.max() < REL and racc.max() < REL
