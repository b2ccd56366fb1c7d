"""The oracle's three options (pso_set_options: drag, force sign, Euler -- include/psamd.h's config.drag, config.force_sign
and PSAMD_FLAG_EULER) checked WITHOUT using them: every test states the operation a second, independent way -- with the
pinned path of an oracle that never had the setter called, and numpy float32 arithmetic.  CPU only.

These tests hold the oracle to the header; GPU tests that run whole steps with the options on (scripts/fuzz_parity.run_case
takes them as `options=`) can then hold the kernels to the oracle byte for byte."""
import numpy as np

import oracle_py as O
from util import explosion_rng

# an 8^3 grid of 5-unit cells, box [-20, 20)^3; lists of 34 per cell, so that the clump below overflows one
GEO = dict(chunk_factor=2, chunk_dim=4, max_particles_num=8192)
LIFE, KID, DT = 15.0, 1.5, 0.05
N = 2500


def mixed_cloud(seed, births=False):
    """kids (some to the ulp of the threshold), adults, elders (to the ulp of the end of life, and past it), masses from
    0 to 100, coincident pairs, a clump that overflows a cell's list, velocities up to 30 times the clamp and exactly on it"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-19.9, 19.9, (N, 3)).astype(np.float32)
    xyz[:60] = (np.array([7.5, -7.5, 2.5]) + rng.normal(0, 0.6, (60, 3))).astype(np.float32)      # one cell, 60 > 34
    xyz[100:120] = xyz[120:140]                                                                 # coincident pairs
    xyz[140:200] = xyz[200:260] + rng.uniform(-0.2, 0.2, (60, 3)).astype(np.float32)             # pairs inside the collision radius
    age = rng.uniform(0.0, 0.9 * LIFE, N).astype(np.float32)
    ulps = lambda v, k: (np.float32(v).view(np.int32) + k).view(np.float32)
    sel = rng.random(N)
    around = rng.integers(-2, 3, N).astype(np.int32)
    age = np.where(sel < 0.1, ulps(KID, around), age)
    age = np.where((sel >= 0.1) & (sel < 0.2), ulps(LIFE, around), age)
    age = np.where((sel >= 0.2) & (sel < 0.25), rng.uniform(LIFE, 2 * LIFE, N), age).astype(np.float32)
    w = np.where(rng.random(N) < 0.1, 0.0, rng.uniform(1.0, 100.0, N)).astype(np.float32)
    v = rng.uniform(-30.0, 30.0, (N, 3)).astype(np.float32)
    v[300:400] = rng.uniform(-300.0, 300.0, (100, 3)).astype(np.float32)                        # v*t past MAX_DX
    v[400:500] = np.float32(10.0) * rng.choice(np.array([-1.0, 1.0], np.float32), (100, 3))     # exactly at MAX_V
    v[500:600] = 0.0
    # a fertility age that is unique: it travels with the particle through a relocation and names it afterwards
    fert = (rng.uniform(0.3 * LIFE, 0.8 * LIFE, N) if births else 1e6 + np.arange(N)).astype(np.float32)
    return xyz, v, age, w, fert


def system_with(cloud, births_seed=None):
    xyz, v, age, w, fert = cloud
    o = O.System(O.default_config(**GEO))
    ids = o.fill(xyz, age=age, fert_age=fert, w=w)
    p = o.particles
    p["vx"][ids], p["vy"][ids], p["vz"][ids] = v.T
    if births_seed is None:
        o.set_explosions(False)
    else:
        o.set_rng(explosion_rng(births_seed))
    return o


def pairs_of(o):
    """(force4 of the whole sorted order, the slot ids in that order) at the frame just built"""
    total = o.sorted_count()
    f = np.zeros((total, 4), np.float32)
    o.calc_pairs(0, total, f)
    cg = o.cellgrid
    order = np.concatenate([cg[c, 1:1 + cg[c, 0]] for c in range(o.d.num_cells)])
    assert len(order) == total
    return f, order


def negated_without_minus_zero(a):
    """bits of -a, with every -0 turned into +0"""
    bits = a.view(np.uint32) ^ np.uint32(0x80000000)
    return np.where(bits == np.uint32(0x80000000), np.uint32(0), bits)


def test_repulsion_is_the_bit_negation_of_gravity():
    """Round-to-nearest is symmetric: every term of the s = -1 sum is the negated term of the s = +1 sum, so every partial
    sum is the negated partial sum -- except that a sum which starts at +0 can never come out as -0 (x + (-x) = +0,
    +0 + -0 = +0).  The collision scan does not know the sign: flags identical.  Snapshot rows and w: untouched."""
    cloud = mixed_cloud(11)
    plus, minus = system_with(cloud), system_with(cloud)
    minus.set_options(force_sign=-1.0)
    for o in (plus, minus):
        o.init_iframe(); o.build_grid()
    fp, order = pairs_of(plus)
    fm, order_m = pairs_of(minus)
    assert np.array_equal(order, order_m)
    flags = fp[:, 3].view(np.int32)
    assert np.array_equal(flags, fm[:, 3].view(np.int32))
    assert np.array_equal(negated_without_minus_zero(fp[:, :3]), fm[:, :3].view(np.uint32))
    assert not (fp[:, :3].view(np.uint32) == np.uint32(0x80000000)).any()
    # the cloud is what it claims: all three flags, kids and massless adults among the flag-0 entries, real forces
    t = plus.tdata[order]
    assert {0, 1, 2} <= set(flags.tolist())
    keep = flags == 0
    assert (t["age"][keep] < np.float32(KID)).sum() > 50 and not fp[keep & (t["age"] < np.float32(KID)), :3].any()
    assert ((t["w"] == 0) & (t["age"] >= np.float32(KID)) & keep).sum() > 20
    assert np.abs(fp[keep, :3]).max() > 1.0 and len(set(t["w"][keep].tolist())) > 100
    assert plus.tdata.tobytes() == minus.tdata.tobytes() and plus.particles.tobytes() == minus.particles.tobytes()
    assert (minus.tdata["w"] >= 0).all()
    plus.close(); minus.close()


def test_drag_is_the_undragged_step_given_a_minus_kv():
    """The drag oracle's step against an oracle WITHOUT drag that is handed a' = a - float32(k)*v (numpy float32: two
    roundings) as the force record of every flag-0 entry: the pinned apply_forces integrates with what it is given and
    stores it.  Every byte of particles, QUEUE_INFO and queue, six steps, births on."""
    k = 0.8
    cloud = mixed_cloud(12, births=True)
    a, b = system_with(cloud, births_seed=77), system_with(cloud, births_seed=77)
    a.set_options(drag=k)
    seen_fused_difference = 0
    for step in range(6):
        a.step(1)
        b.init_iframe(); b.build_grid()
        f, order = pairs_of(b)
        p = b.particles
        v = np.stack([p["vx"][order], p["vy"][order], p["vz"][order]], 1)
        keep = f[:, 3].view(np.int32) == 0
        kv = np.float32(k) * v
        assert kv.dtype == np.float32
        f2 = f.copy()
        f2[keep, :3] = f[keep, :3] - kv[keep]
        # how many entries a fused a - k*v (one rounding) would get wrong: the test can tell the two apart
        fused = (f[keep, :3].astype(np.float64) - np.float64(np.float32(k)) * v[keep].astype(np.float64)).astype(np.float32)
        seen_fused_difference += int((fused.view(np.uint32) != f2[keep, :3].view(np.uint32)).sum())
        b.apply_forces(f2)
        b.advance_step()
        assert a.particles.tobytes() == b.particles.tobytes(), "particles differ at step %d" % (step + 1)
        assert a.queue_info.tobytes() == b.queue_info.tobytes() and a.queue.tobytes() == b.queue.tobytes(), "queues differ at step %d" % (step + 1)
    c = a.counters
    assert c == b.counters
    assert c["integrated"] > 1000 and c["births"] > 0 and c["relocations"] > 0 and c["survives"] > 0 and c["deaths_collision"] > 0
    assert seen_fused_difference > 100
    # the stored acceleration is a' (a kid feels no force and keeps -k*v)
    live = a.particles[a.particles["cell"] >= 0]
    assert np.abs(live["ax"]).max() > 0
    a.close(); b.close()


def test_euler_changes_the_position_update_and_nothing_else():
    """One step from one state with and without the switch.  Velocity, acceleration, age and flags: identical slot for
    slot wherever neither run moved the particle to another slot.  Position of an integrated particle that did not wrap:
    x + clamp(float32(v*t)) in numpy, found after the step by its (unique) fertility age."""
    cloud = mixed_cloud(13)
    xyz, v, age, w, fert = cloud
    ref, eul, probe = system_with(cloud), system_with(cloud), system_with(cloud)
    eul.set_options(euler=True)
    probe.init_iframe(); probe.build_grid()
    f, order = pairs_of(probe)
    before = probe.particles.copy()
    ref.step(1); eul.step(1)
    pr, pe = ref.particles, eul.particles
    stayed = (before["cell"] >= 0) & (pr["cell"] >= 0) & (pe["cell"] >= 0) & \
             (pr["fertility_age"] == before["fertility_age"]) & (pe["fertility_age"] == before["fertility_age"])
    assert stayed.sum() > 1000
    for name in ("vx", "vy", "vz", "ax", "ay", "az", "age", "w", "fertility_age"):
        assert np.array_equal(pr[name][stayed].view(np.uint32), pe[name][stayed].view(np.uint32)), name
    assert np.array_equal(pr["is_parent"][stayed], pe["is_parent"][stayed])
    assert ref.counters["integrated"] == eul.counters["integrated"] and ref.counters["survives"] == eul.counters["survives"]
    assert pr[stayed].tobytes() != pe[stayed].tobytes()              # ... and the positions do differ: 0.5*a*t*t is gone

    slots = order[f[:, 3].view(np.int32) == 0]                       # the integrated ones, by slot before the step
    t, lim = np.float32(DT), np.float32(5.0)
    want = {}
    for ax_name, v_name in (("x", "vx"), ("y", "vy"), ("z", "vz")):
        dx = before[v_name][slots] * t
        assert dx.dtype == np.float32
        with np.errstate(invalid="ignore"):
            dx = np.where(np.abs(dx) > lim, lim * (dx / np.abs(dx)), dx).astype(np.float32)
        want[ax_name] = before[ax_name][slots] + dx
    inside = np.ones(len(slots), bool)
    for ax_name, sgn in (("x", 1.0), ("y", -1.0), ("z", -1.0)):
        i = np.floor(sgn * want[ax_name].astype(np.float64) / 5.0) + 4
        inside &= (i >= 0) & (i < 8)
    where = {fa: s for s, fa in enumerate(pe["fertility_age"].tolist()) if pe["cell"][s] >= 0}
    now = np.array([where[fa] for fa in before["fertility_age"][slots].tolist()])
    assert inside.sum() > 1000 and (~inside).sum() > 10
    for ax_name in ("x", "y", "z"):
        assert np.array_equal(pe[ax_name][now][inside].view(np.uint32), want[ax_name][inside].view(np.uint32)), ax_name
    # the clamp really acted on the shortened dx, and some of those particles changed segment
    vmag = np.abs(np.stack([before["vx"][slots], before["vy"][slots], before["vz"][slots]], 1))
    assert (vmag * t > lim).any(axis=1).sum() > 20 and (vmag == np.float32(10.0)).all(axis=1).sum() > 20
    assert eul.counters["relocations"] > 100
    for o in (ref, eul, probe):
        o.close()


def test_untouched_setter_and_neutral_values_are_the_pinned_path():
    """(0, +1, off) handed to the setter, and 0 as the sign (psamd.h: "0 reads as +1"), change no byte of four steps"""
    cloud = mixed_cloud(14, births=True)
    a, b, c = (system_with(cloud, births_seed=5) for _ in range(3))
    b.set_options(drag=0.0, force_sign=1.0, euler=False)
    c.set_options(force_sign=0.0)
    for o in (a, b, c):
        o.step(4)
    for o in (b, c):
        assert o.particles.tobytes() == a.particles.tobytes() and o.queue.tobytes() == a.queue.tobytes()
        assert o.queue_info.tobytes() == a.queue_info.tobytes() and o.counters == a.counters
    for o in (a, b, c):
        o.close()


def test_the_option_slice_is_what_it_claims():
    """CPU: the campaign cases test_gpu_extras_steps.py runs with the options on are the ones its comments describe"""
    import particlesystem_amd as ps
    from test_gpu_extras_steps import ALL, SLICE, case_of
    cases = [(case_of(s, i), o, g) for s, i, o, g in SLICE]
    assert all(c["steps"] <= 6 for c, _, _ in cases)
    assert all(c["n"] <= 12000 for (c, _, _), (s, i, _, _) in zip(cases, SLICE) if (s, i) != (3303, 25))
    assert case_of(3303, 25)["desc"].startswith("n=40000 G=16 half=39.9 vmax=60 births=1 masses=0 world=2 cuts=None interior=1")
    assert {c["world"] for c, _, _ in cases} == {1, 2, 3, 4, 8}
    one = [(c, o, g) for c, o, g in cases if c["world"] == 1]
    grid = lambda c: c["over"].get("chunk_factor", 4) * c["over"].get("chunk_dim", 4)
    assert any(grid(c) == 16 and o is ALL for c, o, _ in one) and any(grid(c) % 2 and o is ALL for c, o, _ in one)
    assert any(c["births"] and o is ALL for c, o, _ in one) and any(c["reupload"] and o is ALL for c, o, _ in one)
    assert any(g and o is ALL for _, o, g in one)
    assert sorted(len(o) for _, o, _ in one if o is not ALL) == [1, 1, 1]                 # drag, repulsion, Euler alone
    assert sum(1 for c, _, _ in cases if c["v"] is not None and np.isnan(c["v"]).any()) >= 3
    assert any(c["w"] is not None and (c["w"] == 0).any() for c, _, _ in cases)
    slabs = [(c, o, g) for c, o, g in cases if c["world"] > 1]
    assert all(o is ALL for _, o, _ in slabs)
    assert 2 * sum(1 for _, _, g in slabs if g) == len(slabs)
    assert any(c["interior"] for c, _, _ in slabs)
    for w in (2, 3, 4, 8):
        assert any(c["world"] == w and not c["cuts"] for c, _, _ in slabs), w
    lends = 0
    for c, _, _ in slabs:
        if c["cuts"]:
            plans = [ps.slab_plan(ps.default_config(rank=r, world=c["world"], cuts=c["cuts"], **c["over"])) for r in range(c["world"])]
            lends += any(p.lentout_hi > p.lentout_lo for p in plans)
    assert lends >= 2


def test_the_edge_cloud_is_what_it_claims_and_the_exact_path_has_its_yardstick():
    """CPU: the cloud test_gpu_fast.py judges fast math on -- kids, elders, massless adults, coincident pairs, one cell at
    its list capacity and one 40 past it, all three flags -- and the figure fast math is judged against: the worst
    deviation of the exact path's fp32 serial sum (the oracle) from the fp64 re-sum, relative to S_i = sum |term_ij|.
    Printed; DESIGN.md section 5 quotes 7.7e-7 (16^3 cells) and 7.1e-7 (15^3)."""
    import particlesystem_amd as ps
    import test_gpu_fast as T
    from util import oracle_cfg_from
    for grid, over in sorted(T.GRIDS.items()):
        o = O.System(oracle_cfg_from(ps.default_config(flags=ps.FLAG_FAST_MATH, **over)))
        T.fill_both(None, o, T.edge_cloud(over))
        n_dev, idx = T.device_order(o)
        o.init_iframe(); o.build_grid()
        total = o.sorted_count()
        assert len(idx) == total and n_dev - total == 40 == o.counters["cell_overflow_kills"]
        assert (o.cellgrid[:, 0] == o.d.max_per_cell).sum() == 2 and o.cellgrid[:, 0].max() == o.d.max_per_cell
        want = np.zeros((total, 4), np.float32)
        o.calc_pairs(0, total, want)
        flags = want[:, 3].view(np.int32)
        assert min((flags == k).sum() for k in (0, 1, 2)) > 100
        order = np.concatenate([o.cellgrid[c, 1:1 + o.cellgrid[c, 0]] for c in range(o.d.num_cells)])
        t = o.tdata[order]
        assert ((flags == 0) & (t["age"] < np.float32(1.5))).sum() > 500
        assert ((flags == 0) & (t["age"] >= np.float32(1.5)) & (t["w"] == 0)).sum() > 100
        _, _, judged, yard = T.exact_path_yardstick(o, want, order)
        print("edge cloud %s: exact path (oracle) max |a - a64| / S over %d flag-0 adults: %.3g" % (grid, judged.sum(), yard))
        # n terms added serially in fp32 cannot be further than n * 2^-24 of sum |term| from the exact sum
        assert judged.sum() > 5000 and 0 < yard < 27 * o.d.max_per_cell * 2.0 ** -24
        o.close()
