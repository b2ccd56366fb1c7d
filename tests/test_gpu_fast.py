"""PSAMD_FLAG_FAST_MATH (fused multiply-adds + the hardware reciprocal square root in the
pair loop) is the one mode that is not bit-exact.  Tolerance, stated here: the
acceleration vector of every particle within REL_TOL = 1e-5 of the oracle's, relative to its
norm -- BASELINE.json's bar -- collision flags identical.  Checked at 4 and 32 particles per
cell on whole clouds and, in test_fast_math_at_the_benchmark_density, at the benchmark's own
256 per cell (N = 2^20, ~6900-term sums) on windows of the sorted order, with an fp64 re-sum
of the same terms beside it: the reference's own serial fp32 sum is itself ~1e-5 away from
that, so both deviations are printed."""
import numpy as np
import pytest

import oracle_py as O
import particlesystem_amd as ps
from util import assert_same_particles, cloud, explosion_rng, oracle_cfg_from

pytestmark = pytest.mark.gpu
REL_TOL = 1e-5


@pytest.mark.parametrize("n,seed", [(1 << 14, 3), (1 << 17, 4)])
def test_fast_math_pair_pass_within_tolerance(n, seed):
    xyz = cloud(n, seed)
    rng = np.random.default_rng(seed)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    cfg = ps.default_config(flags=ps.FLAG_FAST_MATH)
    g = ps.ParticleSystem(cfg)
    o = O.System(oracle_cfg_from(cfg))
    g.fill_particles(xyz, age=age, fert_age=1e6)
    o.fill(xyz, age=age, fert_age=1e6)
    g.init_iframe(); g.build_grid(); g.calc_forces_pairs()
    o.init_iframe(); o.build_grid()
    total = o.sorted_count()
    want = np.zeros((total, 4), np.float32)
    o.calc_pairs(0, total, want)
    got = g.download_force4(0, total)
    assert np.array_equal(got[:, 3].view(np.int32), want[:, 3].view(np.int32))
    keep = want[:, 3].view(np.int32) == 0
    a, b = got[keep, :3].astype(np.float64), want[keep, :3].astype(np.float64)
    rel = np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-30)
    print("fast-math max relative deviation of |a|: %.3g (n=%d)" % (rel.max(), n))
    assert rel.max() < REL_TOL
    g.calc_forces_apply()


def fp64_resum(o, cells, with_scale=False):
    """acceleration of every particle of `cells` from all bodies of the 27-cell stencil,
    accumulated in float64 (same terms as bodyBodyInteraction, no fp32 rounding)
    with_scale: also S_i = sum over j of |term_ij| (the norm of every term), what the rounding error of the sum scales
    with -- on a clump the terms cancel and |a| says nothing about it; returns (accelerations, scales)"""
    import ctypes as C
    cg, t, d = o.cellgrid, o.tdata, o.d
    out, scale = {}, {}
    n27 = (C.c_int * 27)()
    for c in cells:
        ids = cg[c, 1:1 + cg[c, 0]]
        k = O.lib().pso_fill_cells(C.byref(d), int(c), n27)
        nb = np.concatenate([cg[n27[i], 1:1 + cg[n27[i], 0]] for i in range(k)])
        me, ot = t[ids], t[nb]
        r = np.stack([ot[f].astype(np.float64)[None, :] - me[f].astype(np.float64)[:, None] for f in ("x", "y", "z")], 2)
        d2 = (r * r).sum(2) + 0.2
        s = np.where((ot["age"] < 1.5)[None, :] | (nb[None, :] == ids[:, None]), 0.0, ot["w"].astype(np.float64)[None, :] / (d2 * np.sqrt(d2)))
        acc = (r * s[:, :, None]).sum(1)
        for i, pid in enumerate(ids):
            out[int(pid)] = acc[i]
        if with_scale:
            S = (np.sqrt((r * r).sum(2)) * s).sum(1)
            for i, pid in enumerate(ids):
                scale[int(pid)] = S[i]
    return (out, scale) if with_scale else out


def test_fast_math_at_the_benchmark_density():
    """bench.py's `within_tolerance_mode` is quoted at N = 2^20 in the default box: test it there."""
    n = 1 << 20
    cfg = ps.default_config(flags=ps.FLAG_FAST_MATH)
    g = ps.ParticleSystem(cfg)
    xyz = g.uniform_cloud(n, 2026)
    rng = np.random.default_rng(2026)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    o = O.System(oracle_cfg_from(cfg))
    g.fill_particles(xyz, age=age, fert_age=1e6)
    o.fill(xyz, age=age, fert_age=1e6)
    g.init_iframe(); g.build_grid(); g.calc_forces_pairs()
    o.init_iframe(); o.build_grid()
    total = o.sorted_count()
    start = np.concatenate([[0], np.cumsum(o.cellgrid[:, 0])])
    worst, worst64_fast, worst64_ref = 0.0, 0.0, 0.0
    f = np.zeros((total, 4), np.float32)
    for c0 in (0, 2183, 4070):                      # a corner run, the middle, the far end: 12 cells each
        cells = np.arange(c0, c0 + 12)
        lo, hi = int(start[c0]), int(start[c0 + 12])
        o.calc_pairs(lo, hi, f)
        got = g.download_force4(lo, hi - lo)
        want = f[lo:hi]
        assert np.array_equal(got[:, 3].view(np.int32), want[:, 3].view(np.int32)), "collision flags differ"
        keep = want[:, 3].view(np.int32) == 0
        ids = np.concatenate([o.cellgrid[c, 1:1 + o.cellgrid[c, 0]] for c in cells])
        kid = o.tdata["age"][ids] < 1.5
        keep &= ~kid
        a, b = got[keep, :3].astype(np.float64), want[keep, :3].astype(np.float64)
        rel = np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-30)
        worst = max(worst, rel.max())
        ex = fp64_resum(o, cells)
        e = np.array([ex[int(i)] for i in ids[keep]])
        ne = np.maximum(np.linalg.norm(e, axis=1), 1e-30)
        worst64_fast = max(worst64_fast, (np.linalg.norm(a - e, axis=1) / ne).max())
        worst64_ref = max(worst64_ref, (np.linalg.norm(b - e, axis=1) / ne).max())
    print("N=2^20, 256 per cell: fast-math vs oracle max rel |da|/|a| = %.3g; vs fp64 re-sum: fast %.3g, "
          "reference fp32 serial sum %.3g" % (worst, worst64_fast, worst64_ref))
    assert worst < REL_TOL
    g.calc_forces_apply()
    g.close(); o.close()


# ---- fast math where kernels break -------------------------------------------------------------------------------------------
# Fast math swaps correctly rounded operations (1/2 ulp each) for fma and the hardware rsq (<= 1 ulp): against the fp64
# re-sum of the same terms, and relative to S_i = sum_j |term_ij|, it may deviate up to SLACK times what the exact path's
# own fp32 serial sum (the oracle) deviates on the same cloud.
SLACK = 4.0
GRIDS = {"G16": {}, "G15": {"chunk_factor": 3, "chunk_dim": 5}}


def edge_cloud(over, seed=501, n_bg=10000, births=False):
    """~12 000 particles: kids (ages one ulp either side of the threshold among them), elders (to the ulp of the end of
    life and past it), masses from 0 to 100 (adults of mass 0), coincident pairs, a clump that fills one cell exactly to
    MAX_PARTICLES_PER_CELL and another past it, particles on cell faces.  Returns xyz, v, age, w, fert."""
    cap = O.derive(O.default_config(**over)).max_per_cell
    G = over.get("chunk_factor", 4) * over.get("chunk_dim", 4)
    rng = np.random.default_rng(seed)
    lo, hi = -(G // 2) * 5.0 + 0.1, (G - G // 2) * 5.0 - 0.1            # the box along +x, -y, -z (an odd grid is not centred)
    u = rng.uniform(lo, hi, (n_bg, 3))
    m = n_bg // 10                                                        # on cell faces (the face belongs to the upper cell)
    rows, axis = np.arange(m), rng.integers(0, 3, m)
    u[rows, axis] = np.clip(np.round(u[rows, axis] / 5.0) * 5.0, lo, hi)
    centres = np.array([[12.5, 7.5, -17.5], [-12.5, -7.5, 2.5]])
    for centre in centres:                                                # the two clump cells hold their clumps only
        u = u[(np.floor(u / 5.0) != np.floor(centre / 5.0)).any(axis=1)]
    full = centres[0] + rng.uniform(-2.4, 2.4, (cap, 3))                  # exactly the capacity
    over_full = centres[1] + rng.uniform(-2.4, 2.4, (cap + 40, 3))        # 40 past it
    u = np.concatenate([u, full, over_full])
    u[200:260] = u[260:320]                                               # coincident pairs
    xyz = (u * np.array([1.0, -1.0, -1.0])).astype(np.float32)
    n = len(xyz)
    life, kid = 15.0, 1.5
    ulps = lambda v, k: (np.float32(v).view(np.int32) + k).view(np.float32)
    age = rng.uniform(0.0, 0.9 * life, n).astype(np.float32)
    sel = rng.random(n)
    around = rng.integers(-1, 2, n).astype(np.int32)
    age = np.where(sel < 0.08, ulps(kid, around), age)
    age = np.where((sel >= 0.08) & (sel < 0.14), ulps(life, around), age)
    age = np.where((sel >= 0.14) & (sel < 0.18), rng.uniform(life, 2 * life, n), age).astype(np.float32)
    w = np.where(rng.random(n) < 0.08, 0.0, rng.uniform(1.0, 100.0, n)).astype(np.float32)
    v = rng.uniform(-40.0, 40.0, (n, 3)).astype(np.float32)
    fert = (rng.uniform(0.3 * life, 0.8 * life, n) if births else 1e6 + np.arange(n)).astype(np.float32)
    return xyz, v, age, w, fert


def fill_both(g, o, cloud):
    xyz, v, age, w, fert = cloud
    ids = o.fill(xyz, age=age, fert_age=fert, w=w)
    p = o.particles
    p["vx"][ids], p["vy"][ids], p["vz"][ids] = v.T
    if g is not None:
        assert np.array_equal(g.fill_particles(xyz, age=age, fert_age=fert, w=w, vxyz=v), ids)
    return ids


def device_order(o):
    """Call BEFORE the oracle builds its grid.  The device's sorted order keeps a cell's entries past the list capacity
    (their records read as zero: the cell-overflow rule resets those particles); the oracle's order does not have them.
    Returns (length of the device's order, for every entry of the oracle's order its index in the device's)."""
    p, d = o.particles, o.d
    live = (p["cell"] >= 0) & (p["cell"] < d.num_cells)
    raw = np.bincount(p["cell"][live], minlength=d.num_cells)
    start = np.concatenate([[0], np.cumsum(raw)])
    kept = np.minimum(raw, d.max_per_cell)
    idx = np.concatenate([start[c] + np.arange(kept[c]) for c in np.nonzero(kept)[0]])
    return int(start[-1]), idx


def exact_path_yardstick(o, want, order):
    """(S_i and the fp64 acceleration of every entry of the order, the oracle's own worst deviation over the flag-0 adults)"""
    cells = np.nonzero(o.cellgrid[:, 0])[0]
    ex, sc = fp64_resum(o, cells, with_scale=True)
    e = np.array([ex[int(i)] for i in order])
    S = np.array([sc[int(i)] for i in order])
    judged = (want[:, 3].view(np.int32) == 0) & (o.tdata["age"][order] >= np.float32(1.5)) & (S > 0)
    dev = np.linalg.norm(want[judged, :3].astype(np.float64) - e[judged], axis=1) / S[judged]
    return e, S, judged, float(dev.max())


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_fast_math_pair_pass_on_the_edge_cloud(grid):
    """Flags identical with the oracle for EVERY entry (the cloud has all three, hundreds of each); kids' records zero;
    flag-0 adults within SLACK times the exact path's own deviation, both relative to S_i against the fp64 re-sum.
    Measured: see the printed line."""
    over = GRIDS[grid]
    cfg = ps.default_config(flags=ps.FLAG_FAST_MATH, **over)
    g = ps.ParticleSystem(cfg)
    o = O.System(oracle_cfg_from(cfg))
    fill_both(g, o, edge_cloud(over))
    n_dev, idx = device_order(o)
    g.init_iframe(); g.build_grid(); g.calc_forces_pairs()
    o.init_iframe(); o.build_grid()
    total = o.sorted_count()
    assert len(idx) == total and n_dev - total == 40 == o.counters["cell_overflow_kills"]
    assert o.cellgrid[:, 0].max() == o.d.max_per_cell and (o.cellgrid[:, 0] == o.d.max_per_cell).sum() == 2
    want = np.zeros((total, 4), np.float32)
    o.calc_pairs(0, total, want)
    raw = g.download_force4(0, n_dev)
    got = raw[idx]
    holes = np.ones(n_dev, bool); holes[idx] = False
    assert not raw[holes].any()
    flags = want[:, 3].view(np.int32)
    assert np.array_equal(got[:, 3].view(np.int32), flags), "collision flags differ"
    assert min((flags == 0).sum(), (flags == 1).sum(), (flags == 2).sum()) > 100
    order = np.concatenate([o.cellgrid[c, 1:1 + o.cellgrid[c, 0]] for c in range(o.d.num_cells)])
    t = o.tdata[order]
    kids = (flags == 0) & (t["age"] < np.float32(1.5))
    assert kids.sum() > 500 and not got[kids, :3].any()
    assert ((flags == 0) & (t["age"] >= np.float32(1.5)) & (t["w"] == 0)).sum() > 100          # massless adults feel the others
    e, S, judged, yard = exact_path_yardstick(o, want, order)
    dev = np.linalg.norm(got[judged, :3].astype(np.float64) - e[judged], axis=1) / S[judged]
    print("edge cloud %s: max |a - a64| / S over %d flag-0 adults: fast math %.3g, exact path (oracle) %.3g, allowed %.3g" %
          (grid, judged.sum(), dev.max(), yard, SLACK * yard))
    assert judged.sum() > 5000 and dev.max() <= SLACK * yard
    g.calc_forces_apply()
    # repulsion in fast mode: fma and rsq round symmetrically too, so every partial sum is the negated one; a sum that
    # starts at +0 never ends at -0.  (A kernel that took a negative mass for a kid's would leave zeros here.)
    r = ps.ParticleSystem(ps.default_config(flags=ps.FLAG_FAST_MATH, force_sign=-1.0, **over))
    fill_both(r, O.System(oracle_cfg_from(cfg)), edge_cloud(over))
    r.init_iframe(); r.build_grid(); r.calc_forces_pairs()
    rep = r.download_force4(0, n_dev)[idx]
    r.calc_forces_apply()
    assert np.array_equal(rep[:, 3].view(np.int32), flags)
    neg = got[flags == 0, :3].view(np.uint32) ^ np.uint32(0x80000000)
    neg = np.where(neg == np.uint32(0x80000000), np.uint32(0), neg)
    assert np.array_equal(rep[flags == 0, :3].view(np.uint32), neg) and np.abs(rep[judged, :3]).max() > 0
    g.close(); r.close(); o.close()


def test_fast_math_apply_is_exact_given_the_forces():
    """Everything after the pair pass is the exact path's: the oracle's apply_forces, handed the force records the GPU
    computed in fast mode, leaves the bytes the GPU's calc_forces_apply leaves -- particles and queues, 4 steps, births on.
    With the pairs within tolerance (above), that pins the whole fast-mode step."""
    seed = 4242
    cfg = ps.default_config(flags=ps.FLAG_FAST_MATH | ps.FLAG_EXPLOSIONS, seed=seed)
    g = ps.ParticleSystem(cfg)
    o = O.System(oracle_cfg_from(cfg))
    o.set_rng(explosion_rng(seed))
    fill_both(g, o, edge_cloud({}, seed=502, births=True))
    for step in range(4):
        n_dev, idx = device_order(o)
        g.init_iframe(); g.build_grid(); g.calc_forces_pairs()
        o.init_iframe(); o.build_grid()
        assert len(idx) == o.sorted_count()
        f = np.ascontiguousarray(g.download_force4(0, n_dev)[idx])
        o.apply_forces(f)
        o.advance_step()
        g.calc_forces_apply()
        assert_same_particles(g.download_particles(), o.particles, "fast-mode apply, step %d" % (step + 1))
        qi, q = g.download_queues()
        assert qi.tobytes() == o.queue_info.tobytes() and np.array_equal(q, o.queue), "queues differ at step %d" % (step + 1)
    c = o.counters
    assert c["births"] > 0 and c["relocations"] > 0 and c["survives"] > 0 and c["deaths_collision"] > 0 and c["integrated"] > 5000
    g.close(); o.close()


def fast_state_after(steps, graphs=False, world=1, cuts=None, interior=False):
    from particlesystem_amd.slab import merge_owned, step_local
    xyz, v, age, w, fert = edge_cloud({}, seed=503)
    extra = dict(cuts=cuts) if cuts else {}
    ranks = [ps.ParticleSystem(ps.default_config(flags=ps.FLAG_FAST_MATH, rank=r, world=world, **extra)) for r in range(world)]
    for g in ranks:
        g.fill_particles(xyz, age=age, fert_age=fert, w=w, vxyz=v)
        if graphs:
            g.set_graphs(True)
    out = []
    for _ in range(steps):
        if world == 1:
            ranks[0].step(1)
        else:
            step_local(ranks, overlap_interior=interior)
        plans = [g.slab_plan() for g in ranks]
        qs = [g.download_queues() for g in ranks]
        if world == 1:
            out.append((ranks[0].download_particles(), qs[0][0], qs[0][1]))
        else:
            out.append((merge_owned([g.download_particles() for g in ranks], plans),
                        merge_owned([x[0] for x in qs], plans, "records"), merge_owned([x[1] for x in qs], plans)))
    lends = any(p.lentout_hi > p.lentout_lo for p in plans)
    if graphs:
        assert sum(g.graph_stats()[0] for g in ranks) > 0
    for g in ranks:
        g.close()
    return out, lends


_fast_one = []


def fast_one_gpu():
    if not _fast_one:
        _fast_one.append(fast_state_after(4)[0])
    return _fast_one[0]


def assert_same_states(a, b, what):
    for k, ((pa, qia, qa), (pb, qib, qb)) in enumerate(zip(a, b)):
        assert_same_particles(pa, pb, "%s, step %d" % (what, k + 1))
        assert qia.tobytes() == qib.tobytes() and np.array_equal(qa, qb), "%s: queues differ at step %d" % (what, k + 1)


def test_fast_math_gives_the_same_bytes_twice_and_with_graphs():
    one = fast_one_gpu()
    assert_same_states(fast_state_after(4)[0], one, "fast math, second run")
    assert_same_states(fast_state_after(4, graphs=True)[0], one, "fast math, graphs on")
    live = one[-1][0][one[-1][0]["cell"] >= 0]
    assert len(live) > 5000 and np.abs(live["ax"]).max() > 0


@pytest.mark.parametrize("world,cuts,interior", [(2, [0, 7, 16], False), (4, None, True)], ids=["two-slabs-cuts-0-7-16", "four-slabs-interior"])
def test_fast_math_union_of_slabs_equals_one_gpu(world, cuts, interior):
    """the fast kernel on halo cells, on lent layers and on the interior pass: the same sums in the same order as on one
    GPU, every byte, 4 steps"""
    got, lends = fast_state_after(4, world=world, cuts=cuts, interior=interior)
    # (by the plan it is the balanced four that lend: their cuts at 4, 8, 12 fall inside the segment groups {3, 4}, {7, 8},
    # {11, 12}; a cut at 7 is group-aligned.  Between the two worlds the fast kernel runs on halo cells, a lent layer and
    # the interior pass.)
    assert lends == (world == 4)
    assert_same_states(got, fast_one_gpu(), "fast math, %d slabs" % world)


def test_fast_math_all_pairs_against_an_fp64_direct_sum():
    """PSAMD_FLAG_FAST_MATH | PSAMD_FLAG_ALL_PAIRS on a cloud spread over the whole box: the project's 1e-5 of the fp64
    direct sum (the form of test_gpu_extras.py::test_all_pairs_against_an_fp64_direct_sum)"""
    n = 4000
    xyz = cloud(n, 8)
    rng = np.random.default_rng(8)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    age[::17] = 0.5
    g = ps.ParticleSystem(ps.default_config(flags=ps.FLAG_ALL_PAIRS | ps.FLAG_FAST_MATH, collision_radius=1e-6))
    ids = g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    g.init_iframe(); g.build_grid(); g.calc_forces_pairs()
    f = g.download_force4(0, n)
    order = np.concatenate([row[1:1 + row[0]] for row in g.download_cellgrid()])
    g.calc_forces_apply()
    pos = xyz.astype(np.float64)
    kid = age < 1.5
    d = pos[None, :, :] - pos[:, None, :]
    r2 = (d * d).sum(2) + 0.2
    s = np.where(kid[None, :], 0.0, 60.0 / (r2 * np.sqrt(r2)))
    np.fill_diagonal(s, 0.0)
    exact = (d * s[:, :, None]).sum(1)
    where = np.empty(g.sizes.container_size, np.int64)
    where[ids] = np.arange(n)
    idx = where[order]
    got, want = f[:, :3].astype(np.float64), exact[idx]
    assert (f[:, 3].view(np.int32) == 0).all()
    adults = ~kid[idx]
    rel = np.linalg.norm(got[adults] - want[adults], axis=1) / np.linalg.norm(want[adults], axis=1)
    print("fast math + all-pairs vs fp64 direct sum, N=%d: max relative deviation %.3g" % (n, rel.max()))
    assert rel.max() < REL_TOL and not got[~adults].any()
    g.close()
