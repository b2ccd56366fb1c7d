"""Drag, the Euler switch and repulsion (include/psamd.h: config.drag, config.force_sign, PSAMD_FLAG_EULER) on WHOLE STEPS,
against the oracle's restatement of the header (pso_set_options; held to the header on the CPU by test_oracle_extras.py),
every byte after every step: cases the randomised campaigns already drew (scripts/fuzz_parity.py: faces to the ulp,
velocities at the clamp, threshold ages, masses, births, clumps that overflow cells, odd grids, velocities that are not a
number), run with the options on -- one context, reuploads, graphs, and slabs of 2, 3, 4 and 8 ranks with balanced and the
caller's cuts (lent layers: the force record comes back from the rank above and the owner applies the drag), the interior
pass.  Beside them: the T_DATA mirror under repulsion, and all-pairs with the options.

What the toy-input tests of test_gpu_extras.py cannot see and these do: a fused a - k*v (with a = 0 it is -(k*v) either
way), an acc4 left unwritten under drag, a signed w in the T_DATA mirror, a halo message that drops the sign."""
import os
import sys

import numpy as np
import pytest

import particlesystem_amd as ps
from test_gpu_fuzz import CAMPAIGNS
from util import assert_same_particles, oracle_from

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))

pytestmark = pytest.mark.gpu

ALL = dict(drag=0.8, force_sign=-1.0, flags=ps.FLAG_EULER)
DRAG, REPULSION, EULER = dict(drag=0.8), dict(force_sign=-1.0), dict(flags=ps.FLAG_EULER)
# (campaign seed, case index, options, graphs): what the case brings
SLICE = [
    # ---- one context
    (4101, 39, ALL, True),        # G = 16, n = 12 000, births, 5 steps, graphs
    (4101, 37, ALL, False),       # G = 15 (odd), n = 12 000, births, two velocities that are not a number
    (4101, 29, ALL, True),        # G = 15, v up to 300 (MAX_DX clamp on the Euler dx), births, collision radius 1
    (4101, 17, ALL, False),       # eps2 = 1e-20: the generic exact pair kernel (its `w == 0` branch meets negative masses)
    (4103, 53, ALL, False),       # reupload half way; 12 000 in a blob of 12 cells, v up to 300, collision radius 1
    (4101, 9, DRAG, False),       # drag alone: dense blob, births, replay from the snapshot
    (4101, 13, REPULSION, False), # repulsion alone: masses (some zero), births, not-a-number velocities
    (4101, 11, EULER, False),     # Euler alone: v up to 300, masses, reupload
    # ---- slabs
    (3303, 25, ALL, True),        # the find of round 3 (births make a child whose velocity is no number): n = 40 000 as it
                                  # was drawn, 2 slabs, interior pass, graphs
    (4101, 4, ALL, False),        # 2 slabs, cuts [0, 2, 12]: lends layers; masses
    (4101, 5, ALL, True),         # 2 slabs, cuts [0, 14, 16]: lends layers; dense blob, dt 0.2
    (4101, 12, ALL, False),       # 2 slabs, balanced, interior pass
    (4101, 0, ALL, True),         # 3 slabs, balanced, G = 12, births, dt 0.2
    (4101, 6, ALL, False),        # 3 slabs, balanced, G = 20, v up to 300, births, masses
    (4101, 2, ALL, True),         # 4 slabs, balanced, interior pass, dense blob, v up to 300, births
    (4101, 14, ALL, False),       # 4 slabs, balanced, interior pass, masses, not-a-number velocities
    (3303, 23, ALL, False),       # 4 slabs, cuts [0, 5, 8, 10, 12]: lends layers; births
    (4103, 8, ALL, True),         # 4 slabs, cuts [0, 9, 11, 13, 16], interior pass, v up to 300, births
    (4102, 5, ALL, True),         # 8 slabs, balanced, births, not-a-number velocities
    (4102, 6, ALL, False),        # 8 slabs, balanced, interior pass, v up to 300
]
_drawn, _results = {}, {}


def case_of(seed, index):
    """the index-th case of the campaign, as test_gpu_fuzz draws it (one random stream per campaign, in order)"""
    if seed not in _drawn:
        from fuzz_parity import draw_case
        sizes, worlds, max_steps, legacy, _ = CAMPAIGNS[seed]
        rng = np.random.default_rng(seed)
        last = max(i for s, i, _, _ in SLICE if s == seed)
        _drawn[seed] = [draw_case(rng, sizes, max_steps, worlds, nan_draw=not legacy) for _ in range(last + 1)]
    return _drawn[seed][index]


def result_of(k):
    """(run_case's verdict, the oracle's counters) of SLICE[k]; every case runs once"""
    if k not in _results:
        from fuzz_parity import run_case
        seed, index, options, graphs = SLICE[k]
        counters = {}
        res = run_case(case_of(seed, index), 1000 + index, graphs=graphs, options=options, counters_out=counters)
        _results[k] = (res, counters)
    return _results[k]


def option_name(o):
    return "all" if o is ALL else "drag" if o is DRAG else "repulsion" if o is REPULSION else "euler"


@pytest.mark.timeout(300)
@pytest.mark.parametrize("k", range(len(SLICE)), ids=["seed%d-case%d-%s%s" % (s, i, option_name(o), "-graphs" if g else "") for s, i, o, g in SLICE])
def test_campaign_case_with_the_options_equals_the_oracle_byte_for_byte(k):
    res, _ = result_of(k)
    assert res.startswith("ok"), "%s: %s" % (case_of(*SLICE[k][:2])["desc"], res)      # a refusal or a skip tests nothing


@pytest.mark.timeout(900)
def test_the_slice_met_every_event():
    total = {}
    for k in range(len(SLICE)):
        res, counters = result_of(k)
        assert res.startswith("ok"), res
        for name, v in counters.items():
            total[name] = total.get(name, 0) + v
    print("events over the slice:", total)
    for name in ("integrated", "survives", "deaths_collision", "relocations", "births"):
        assert total[name] > 0, (name, total)


def mixed(n, seed, half=39.9):
    """positions, ages with kids among them, masses from 0 to 100"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-half, half, (n, 3)).astype(np.float32)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    age[::13] = 0.5
    w = np.where(rng.random(n) < 0.1, 0.0, rng.uniform(1.0, 100.0, n)).astype(np.float32)
    return xyz, age, w


def test_tdata_mirror_keeps_the_unsigned_mass_under_repulsion():
    """the sign lives in the pair stage's own snapshot (w_eff); the T_DATA rows are the reference's: x, y, z, w, age, id"""
    n = 6000
    xyz, age, w = mixed(n, 61)
    g = ps.ParticleSystem(ps.default_config(force_sign=-1.0))
    o = oracle_from(g.cfg)
    ids = g.fill_particles(xyz, age=age, fert_age=np.float32(1e6), w=w)
    o.fill(xyz, age=age, fert_age=np.float32(1e6), w=w)
    g.init_iframe(); g.build_grid()
    o.init_iframe(); o.build_grid()
    t = g.download_tdata()
    assert t[ids].tobytes() == o.tdata[ids].tobytes()
    assert np.array_equal(t["w"][ids], w) and (t["w"] >= 0).all() and not np.signbit(t["w"]).any()
    assert (w[age >= 1.5] > 0).sum() > 1000
    g.calc_forces()
    o.calc_forces()
    assert_same_particles(g.download_particles(), o.particles, "repulsion, one step")
    assert not np.signbit(g.download_particles()["w"]).any()
    g.close(); o.close()


def pair_pass(g, n):
    g.init_iframe(); g.build_grid(); g.calc_forces_pairs()
    f = g.download_force4(0, n)
    g.calc_forces_apply()
    return f


def test_all_pairs_repulsion_is_the_bit_negation_of_all_pairs_gravity():
    """near and far walk alike: every term negated, every partial sum negated; a sum that starts at +0 never ends at -0"""
    n = 5000
    xyz, age, w = mixed(n, 62)
    f = {}
    for sign in (1.0, -1.0):
        g = ps.ParticleSystem(ps.default_config(flags=ps.FLAG_ALL_PAIRS, force_sign=sign))
        g.fill_particles(xyz, age=age, fert_age=np.float32(1e6), w=w)
        f[sign] = pair_pass(g, n)
        g.close()
    flags = f[1.0][:, 3].view(np.int32)
    assert np.array_equal(flags, f[-1.0][:, 3].view(np.int32))
    keep = flags == 0
    a, b = f[1.0][keep, :3], f[-1.0][keep, :3]
    want = a.view(np.uint32) ^ np.uint32(0x80000000)
    want = np.where(want == np.uint32(0x80000000), np.uint32(0), want)
    assert np.array_equal(want, b.view(np.uint32))
    assert not (a.view(np.uint32) == np.uint32(0x80000000)).any() and np.abs(a).max() > 0
    assert (~a.any(axis=1)).sum() > 300                     # the kids: zero records under either sign


def test_all_pairs_with_the_options_across_two_slabs_equals_one_gpu():
    """the sign travels in the all-gather block's mass, the owner applies drag and Euler: union == one GPU, every byte
    (the oracle has no far field, so one GPU is the yardstick here, as in test_gpu_extras.py)"""
    from particlesystem_amd.slab import merge_owned, step_local
    n = 5000
    xyz, age, w = mixed(n, 63)
    rng = np.random.default_rng(63)
    v = rng.uniform(-60, 60, (n, 3)).astype(np.float32)
    fert = (1e6 + np.arange(n)).astype(np.float32)
    opt = dict(flags=ps.FLAG_ALL_PAIRS | ps.FLAG_EULER, drag=0.8, force_sign=-1.0)
    one = ps.ParticleSystem(ps.default_config(**opt))
    ranks = [ps.ParticleSystem(ps.default_config(rank=r, world=2, **opt)) for r in range(2)]
    for s in [one] + ranks:
        s.fill_particles(xyz, age=age, fert_age=fert, w=w, vxyz=v)
    plans = [g.slab_plan() for g in ranks]
    for step in range(3):
        one.step(1)
        step_local(ranks)
        want = one.download_particles()
        assert_same_particles(merge_owned([g.download_particles() for g in ranks], plans), want, "step %d" % (step + 1))
        qs = [g.download_queues() for g in ranks]
        qi, q = one.download_queues()
        assert merge_owned([x[0] for x in qs], plans, "records").tobytes() == qi.tobytes()
        assert np.array_equal(merge_owned([x[1] for x in qs], plans), q)
    live = want[want["cell"] >= 0]
    assert one.counters["relocations"] > 0 and np.abs(live["ax"]).max() > 0
    for s in [one] + ranks:
        s.close()
