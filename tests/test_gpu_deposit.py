"""The mass on a lattice on the device (psamd_deposit / psamd_deposit_result_get / psamd_download_deposit, deposit.hip).

What pins the arithmetic: the numpy model of tests/deposit_model.py, written from include/psamd.h alone and fed with the frame
the device built (the sorted snapshot and cell_start, read back through psamd_device_view_get).  The model forms the same fp32
terms; the fp64 sums of non-negative terms differ only in their order, so only the last rounding can differ: every voxel
within 1 ulp, a voxel without mass exactly +0, the counts exact, the mass within 2^-40.  Everything else is byte equality: twice
on one frame, through a captured graph, after the pair stage, on every context kind, and a slab world's union against one
context.  Shapes: 8^3 cells and the odd 9^3 (G / 2 rounds down), about 4 000 bodies; slabs on 16^3 with 8 000."""
import ctypes as C

import numpy as np
import pytest
import torch

import deposit_model as D
import particlesystem_amd as ps
from particlesystem_amd import slab
from service_harness import DEV, ERR_INVALID_ARG, ERR_STATE, bits, captured, dev_read, open_frame, state

pytestmark = pytest.mark.gpu

CS = 5.0
GRIDS = {8: dict(max_particles_num=16384, chunk_factor=2, chunk_dim=4),      # lists of 66
         9: dict(max_particles_num=16384, chunk_factor=3, chunk_dim=3),      # lists of 46; G / 2 = 4: the box is not centred
         16: dict(max_particles_num=16384, chunk_factor=4, chunk_dim=4, x_factor=8)}     # lists of 40
QUIET = dict(collision_radius=1e-6, drag=0.0)          # nothing collides
NAN_FILL = 0x7fc0dead                                # what no deposit writes


def snapshot(g):
    """the frame build_grid left on one context: x, y, z, w_eff by sorted index and cell_start"""
    g.synchronize()
    v = g.device_view()
    start = dev_read(v.cell_start, g.sizes.num_cells + 1, np.int32)
    n = int(start[-1])
    x, y, z, w = (dev_read(v.snap_soa + 4 * k * v.sorted_cap, n, np.float32) for k in range(4))
    return x, y, z, w, start


def model(g, snap, refine, exact=False):
    return D.deposit(*snap, g.sizes.grid_dim, CS, g.sizes.max_per_cell, refine, exact=exact)


def rough_cloud(G, cap, seed=3):
    """about 4 000 bodies in cell-axis coordinates q = (-y, x, -z): a uniform cloud; bodies on cell faces and one ulp beside
    them; bodies within h / 2 of the box faces (past the outermost voxel centres of every refine); a clump that overflows one
    cell's list; every 17th a kid, every 29th massless"""
    rng = np.random.default_rng(seed)
    lo, hi = -(G // 2) * CS, (G - G // 2) * CS
    q = [rng.uniform(lo + 0.001, hi - 0.001, (3200, 3))]
    face = rng.uniform(lo + 0.7, hi - 0.7, (300, 3)).astype(np.float32)
    planes = np.float32(CS) * rng.integers(-(G // 2) + 1, G - G // 2, 300).astype(np.float32)
    side = np.arange(300) % 3
    planes = np.where(side == 1, np.nextafter(planes, np.float32(np.inf)), np.where(side == 2, np.nextafter(planes, np.float32(-np.inf)), planes))
    face[np.arange(300), rng.integers(0, 3, 300)] = planes
    q.append(face)
    rim = rng.uniform(lo + 0.001, hi - 0.001, (300, 3))
    d = rng.uniform(0.001, 0.6, 300)
    rim[np.arange(300), rng.integers(0, 3, 300)] = np.where(np.arange(300) % 2 == 0, lo + d, hi - d)
    q.append(rim)
    q.append(np.array([lo + 2 * CS, lo + 3 * CS, lo + 1 * CS]) + rng.uniform(0.05, 4.95, (cap + 12, 3)))      # twelve more than the list holds
    q = np.concatenate(q).astype(np.float32)
    xyz = np.stack([q[:, 1], -q[:, 0], -q[:, 2]], 1)
    n = len(xyz)
    age = np.full(n, 3.0, np.float32)
    age[::17] = 0.5
    w = rng.uniform(20.0, 100.0, n).astype(np.float32)
    w[::29] = 0.0
    return xyz, age, w


def system(G, cloud, flags=0, **over):
    g = ps.ParticleSystem(ps.default_config(flags=flags, **{**GRIDS[G], **QUIET, **over}))
    assert g.sizes.grid_dim == G
    xyz, age, w = cloud
    g.fill_particles(xyz, age=age, w=w, fert_age=np.float32(1e6))
    return g


@pytest.fixture(scope="module")
def clouds():
    return {G: rough_cloud(G, {8: 66, 9: 46}[G]) for G in (8, 9)}


@pytest.fixture(scope="module")
def built(clouds):
    """per grid one context with its frame built -- among the rest a body of infinite mass and, on 8^3, one whose x is no number
    (an upload files such a position under one fixed cell: cell 0 there) -- and the frame read back"""
    made = {}

    def get(G):
        if G not in made:
            g = system(G, clouds[G])
            p = g.download_particles()
            live = np.nonzero(p["cell"] >= 0)[0]
            per_cell = np.bincount(p["cell"][live], minlength=G ** 3)
            calm = (np.abs(p["x"][live]) < 19) & (np.abs(p["y"][live]) < 19) & (np.abs(p["z"][live]) < 19)      # (an upload checks |x| against half the box)
            b = int(live[np.nonzero((p["cell"][live] != 0) & (per_cell[p["cell"][live]] < 20) & calm)[0][7]])     # (not in the clump: it stays listed)
            p["w"][b] = np.inf
            p["age"][b] = 3.0
            g.upload_particles(p[b:b + 1], first=b)
            if G == 8:
                a = int(live[np.nonzero(p["cell"][live] == 0)[0][0]])
                p["x"][a] = np.nan
                g.upload_particles(p[a:a + 1], first=a)
            open_frame(g)
            made[G] = (g, snapshot(g))
        return made[G]
    yield get
    for g, _ in made.values():
        g.close()


# ---- 1. the device against the fp32 model --------------------------------------------------------------------------------------

@pytest.mark.parametrize("refine", D.REFINES)
@pytest.mark.parametrize("G", [8, 9])
def test_device_against_the_model(built, G, refine):
    g, snap = built(G)
    M = G * refine
    want = model(g, snap, refine)
    assert want["skipped"] == (2 if G == 8 else 1) and want["bodies"] > 3800
    counts = np.diff(snap[4])
    assert counts.max() > g.sizes.max_per_cell or g.counters["cell_overflow_kills"] >= 12      # the clump met the list cap
    got, res = g.deposit(refine, result=True)
    assert tuple(got.shape) == (M, M, M)
    gb, wb = bits(got).astype(np.int64), bits(want["rho"]).astype(np.int64)
    ulp = np.abs(gb - wb)
    rel = abs(res["mass"] - want["mass"]) / want["mass"]
    print("%d^3 cells, refine %d: %d voxels with mass of %d, %d differ by 1 ulp, none by more: %s; mass %.9g, relative error %.3g"
          % (G, refine, (wb != 0).sum(), M ** 3, (ulp == 1).sum(), ulp.max() <= 1, res["mass"], rel))
    assert ulp.max() <= 1
    assert (gb[wb == 0] == 0).all(), "a voxel the model has at 0 is not +0"
    assert (res["voxels"], res["bodies"], res["skipped"]) == (M ** 3, want["bodies"], want["skipped"])
    assert rel <= 2.0 ** -40
    assert res["vmax"] == float(got.max().item()) and res == g.deposit_result()
    # the volume is the gravitating mass: the adults' |w|, kids and the two skipped bodies left out, within four roundings a term
    total = float(np.abs(snap[3][np.isfinite(snap[0]) & np.isfinite(snap[3])]).astype(np.float64).sum()) if counts.max() <= g.sizes.max_per_cell else None
    if total is not None:
        assert abs(res["mass"] - total) <= 2.0 ** -21 * total
    # the host form is the same pass
    host, hres = g.download_deposit(refine)
    assert np.array_equal(bits(host), bits(got)) and hres == res
    # accuracy: the plain fp64 form, within the bound of u's rounding (tests/test_deposit_cpu.py derives it for M a power of two;
    # printed here, and held with the factor the odd grid's u needs: |u| < M alone gives 1.75 M 2^-24 an axis)
    exact = model(g, snap, refine, exact=True)
    err, bound = np.abs(want["sums"] - exact["sums"]), 4.0 * M * 2.0 ** -24 * exact["support"]
    print("   fp32 model against the fp64 form: largest error / (4 M 2^-24 mass in reach) %.3g" % (err[bound > 0] / bound[bound > 0]).max())
    assert (err <= 1.75 * bound).all()


# ---- 2. the same bytes twice ---------------------------------------------------------------------------------------------------

def stepped(graphs, steps=3):
    rng = np.random.default_rng(11)
    n = 4000
    g = ps.ParticleSystem(ps.default_config(**GRIDS[8]))
    g.set_graphs(graphs)
    xyz = rng.uniform(-19.9, 19.9, (n, 3)).astype(np.float32)
    g.fill_particles(xyz, age=rng.uniform(0.2, 9.0, n).astype(np.float32), fert_age=np.float32(1e6),
                     vxyz=rng.uniform(-8, 8, (n, 3)).astype(np.float32))
    g.step(steps)
    open_frame(g)
    return g


def state_of(g):
    return [a.tobytes() for a in state(g)]


@pytest.mark.parametrize("refine", D.REFINES)
def test_same_bytes_twice_through_a_graph_and_after_the_pair_stage(refine):
    g = stepped(False)
    before = state_of(g)
    a, ra = g.deposit(refine, result=True)
    b, rb = g.deposit(refine, result=True)
    assert ra["bodies"] > 3000 and np.array_equal(bits(a), bits(b)) and ra == rb
    assert state_of(g) == before, "the deposit touched particles or queues"
    # captured into a caller's graph (nothing is allocated by the call) and replayed
    out2 = torch.full_like(a, float("nan"))
    rec = torch.zeros(C.sizeof(ps.DepositResult), dtype=torch.uint8, device=DEV)
    spec = ps.DepositSpec(refine=refine, out=out2.data_ptr(), capacity=out2.numel(), result_dev=rec.data_ptr())
    with captured(g) as cap:
        rc = g.lib.psamd_deposit(g.h, C.byref(spec))
    assert rc == 0
    cap.launch()
    assert np.array_equal(bits(out2), bits(a)) and ps.DepositResult.from_device(rec).to_dict() == ra
    cap.close()
    # after the pair stage: the same bytes, and the force records are left alone
    g.calc_forces_pairs()
    listed = int(g.download_cellgrid()[:, 0].sum())
    f0, s0 = g.download_force4(0, listed).tobytes(), state_of(g)
    c, rc_ = g.deposit(refine, result=True)
    assert np.array_equal(bits(c), bits(a)) and rc_ == ra
    assert g.download_force4(0, listed).tobytes() == f0 and state_of(g) == s0
    g.calc_forces_apply()
    g.step(1)                                                   # the step goes on
    # with graphs on
    h = stepped(True)
    d, rd = h.deposit(refine, result=True)
    assert h.graph_stats()[0] > 0
    assert np.array_equal(bits(d), bits(a)) and rd == ra
    g.synchronize(); h.synchronize()
    g.close(); h.close()


# ---- 3. every context kind, on one cloud ---------------------------------------------------------------------------------------

KINDS = {"fast math": ps.FLAG_FAST_MATH, "all-pairs": ps.FLAG_ALL_PAIRS, "flat": ps.FLAG_FAR_MONOPOLE, "pyramid": ps.FLAG_FAR_PYRAMID,
         "quadrupole": ps.FLAG_FAR_PYRAMID | ps.FLAG_FAR_QUADRUPOLE}


def test_every_context_kind_returns_the_cutoff_bytes(clouds):
    def run(flags):
        g = system(8, clouds[8], flags)
        open_frame(g)
        out = [g.deposit(k, result=True) for k in D.REFINES]
        g.calc_forces()
        g.synchronize()
        g.close()
        return [(bits(a), r) for a, r in out]
    want = run(0)
    assert all(r["bodies"] > 3800 and r["mass"] > 0 for _, r in want)
    for name, flags in KINDS.items():
        for (a, r), (b, s) in zip(want, run(flags)):
            assert np.array_equal(a, b) and r == s, name


# ---- 4. slabs ------------------------------------------------------------------------------------------------------------------

def slab_cloud(G, n, seed=61):
    rng = np.random.default_rng(seed)
    half = G * 2.5 * 0.9995
    age = rng.uniform(0.2, 9.0, n).astype(np.float32)            # one in seven is a kid
    return dict(xyz=rng.uniform(-half, half, (n, 3)).astype(np.float32), age=age, w=rng.uniform(20.0, 100.0, n).astype(np.float32),
                fert_age=np.float32(1e6), vxyz=rng.uniform(-8, 8, (n, 3)).astype(np.float32))


def union_of(ranks, refine, want, res):
    """every rank's deposit into an array of its own, prefilled: no voxel written twice, every voxel once, the single context's
    bytes; the records merged; the host forms added"""
    M = want.shape[0]
    union = np.full(M ** 3, NAN_FILL, np.uint32)
    recs, hosts = [], []
    for s in ranks:
        out = torch.from_numpy(np.full((M, M, M), NAN_FILL, np.uint32).view(np.float32)).to(DEV)
        got, r = s.deposit(refine, out=out, result=True)
        b = bits(got).ravel()
        wrote = b != NAN_FILL
        assert wrote.sum() == r["voxels"] and (union[wrote] == NAN_FILL).all(), "a voxel was written by two ranks"
        union[wrote] = b[wrote]
        recs.append(r)
        host, hr = s.download_deposit(refine)
        assert hr == r and np.array_equal(bits(host).ravel()[wrote], b[wrote]) and (bits(host).ravel()[~wrote] == 0).all()
        hosts.append(host)
    assert (union != NAN_FILL).all(), "a voxel was written by no rank"
    assert np.array_equal(union, bits(want).ravel()), "the ranks' voxels differ from the single context's"
    merged = ps.merge_deposit(recs)
    assert {k: merged[k] for k in ("voxels", "bodies", "skipped", "vmax")} == {k: res[k] for k in ("voxels", "bodies", "skipped", "vmax")}
    assert abs(merged["mass"] - res["mass"]) <= 2.0 ** -40 * res["mass"], (merged, res)
    assert np.array_equal(bits(sum(hosts[1:], hosts[0])), bits(want))


@pytest.mark.parametrize("world,cuts", [(2, [0, 8, 16]), (2, [0, 7, 16]), (3, None)])
def test_slabs_give_the_single_context_bytes(world, cuts):
    inputs = slab_cloud(16, 8000)
    over = dict(GRIDS[16], **({"cuts": cuts} if cuts else {}))
    one = ps.ParticleSystem(ps.default_config(**GRIDS[16]))
    one.fill_particles(**inputs)
    ranks = [ps.ParticleSystem(ps.default_config(rank=r, world=world, **over)) for r in range(world)]
    plans = [s.slab_plan() for s in ranks]
    print("world %d, cuts %s: lent-in layers %s" % (world, cuts, [(p.lentin_lo, p.lentin_hi) for p in plans]))
    for s in ranks:
        s.fill_particles(**inputs)
    for step in range(2):
        if step:
            one.step(1)
            slab.step_local(ranks)
        open_frame(one)
        slab.to_pairs(ranks)
        for refine in D.REFINES:
            want, res = one.deposit(refine, result=True)
            assert res["voxels"] == (16 * refine) ** 3 and res["bodies"] > 7000
            union_of(ranks, refine, want, res)
        one.calc_forces()
        slab.apply_stage(ranks)
        slab.finish_stage(ranks)
    assert sum(s.live_count() for s in ranks) == one.live_count() > 7000       # the steps went on
    one.close()
    for s in ranks:
        s.close()


def test_a_far_slab_is_served_and_the_step_after_matches_a_run_without_the_call():
    flags = ps.FLAG_FAR_PYRAMID
    inputs = slab_cloud(8, 3000, seed=62)

    def world2():
        ranks = [ps.ParticleSystem(ps.default_config(flags=flags | ps.FLAG_FAR_SLAB, rank=r, world=2, **GRIDS[8])) for r in range(2)]
        for s in ranks:
            s.fill_particles(**inputs)
        return ranks
    one = ps.ParticleSystem(ps.default_config(flags=flags, **GRIDS[8]))
    one.fill_particles(**inputs)
    with_call, without = world2(), world2()
    open_frame(one)
    slab.to_pairs(with_call)
    slab.to_pairs(without)
    for refine in D.REFINES:
        want, res = one.deposit(refine, result=True)
        union_of(with_call, refine, want, res)
    one.calc_forces()
    slab.apply_stage(with_call)
    slab.finish_stage(with_call)
    slab.apply_stage(without)
    slab.finish_stage(without)
    slab.step_local(with_call)
    slab.step_local(without)
    for a, b in zip(with_call, without):
        assert a.download_particles().tobytes() == b.download_particles().tobytes(), "the step after a deposit differs from a run without it"
        qa, qb = a.download_queues(), b.download_queues()
        assert qa[0].tobytes() == qb[0].tobytes() and qa[1].tobytes() == qb[1].tobytes()
    assert sum(s.live_count() for s in with_call) > 2000
    one.synchronize()
    one.close()
    for s in with_call + without:
        s.close()


# ---- 5. window and arguments ---------------------------------------------------------------------------------------------------

def test_window_and_arguments(clouds):
    g = system(8, clouds[8])
    M3 = 16 ** 3                                                  # refine 2
    buf = torch.zeros(M3 + 8, dtype=torch.float32, device=DEV)
    rec = torch.zeros(64, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    good = dict(flags=0, refine=2, out=buf.data_ptr(), capacity=M3, result_dev=rec.data_ptr())

    def call(**kw):
        with g._on_stream(DEV):
            return g.lib.psamd_deposit(g.h, C.byref(ps.DepositSpec(**{**good, **kw})))
    assert call() == ERR_STATE                                    # no frame built
    with pytest.raises(ps.PsamdError) as e:
        g.download_deposit(2)
    assert e.value.status == ERR_STATE
    g.init_iframe()
    assert call() == ERR_STATE
    g.build_grid()
    assert call() == 0
    for bad in (dict(refine=0), dict(refine=3), dict(refine=8), dict(capacity=M3 - 1), dict(flags=1), dict(out=None),
                dict(out=buf.data_ptr() + 2), dict(result_dev=rec.data_ptr() + 4)):
        assert call(**bad) == ERR_INVALID_ARG, bad
    assert g.lib.psamd_deposit(g.h, None) == ERR_INVALID_ARG and g.lib.psamd_deposit_result_get(g.h, None) == ERR_INVALID_ARG
    host = np.zeros(M3, np.float32)
    assert g.lib.psamd_download_deposit(g.h, 2, None, M3, None) == ERR_INVALID_ARG
    assert g.lib.psamd_download_deposit(g.h, 3, host.ctypes.data_as(C.c_void_p), M3, None) == ERR_INVALID_ARG
    assert g.lib.psamd_download_deposit(g.h, 2, host.ctypes.data_as(C.c_void_p), M3 - 1, None) == ERR_INVALID_ARG
    assert call() == 0                                            # the refusals left the context usable
    assert ps.DepositResult.from_device(rec[:C.sizeof(ps.DepositResult)]).to_dict() == g.deposit_result()     # result_dev and the own record agree
    assert g.deposit_result()["voxels"] == M3 and call(result_dev=None) == 0 and g.deposit_result()["voxels"] == M3
    assert g.lib.psamd_download_deposit(g.h, 2, host.ctypes.data_as(C.c_void_p), M3, None) == 0
    assert np.array_equal(bits(host), bits(buf[:M3]))
    assert (bits(buf[M3:]) == 0).all()                            # nothing past M^3
    g.calc_forces()
    assert call() == ERR_STATE                                    # the frame has ended
    g.step(1)
    open_frame(g)
    assert call() == 0
    g.synchronize()
    g.close()


def test_a_slab_outside_its_window_is_refused():
    inputs = slab_cloud(16, 4000)
    ranks = [ps.ParticleSystem(ps.default_config(rank=r, world=2, cuts=[0, 7, 16], **GRIDS[16])) for r in range(2)]
    for s in ranks:
        s.fill_particles(**inputs)

    def refused(s):
        with pytest.raises(ps.PsamdError) as e:
            s.deposit(1)
        return e.value.status == ERR_STATE
    assert all(refused(s) for s in ranks)
    for s in ranks:
        s.slab_build()
    assert all(refused(s) for s in ranks)                        # before slab_pairs: the halos are not in yet
    slab.gather(ranks, slab.STATUS_OUT, slab.STATUS_IN)
    slab.deliver(ranks, "halo")
    for s in ranks:
        s.slab_pairs()
    assert sum(s.deposit(1, result=True)[1]["voxels"] for s in ranks) == 16 ** 3
    slab.apply_stage(ranks)
    assert all(refused(s) for s in ranks)                        # after slab_apply
    slab.deliver(ranks, "xfer")
    for s in ranks:
        s.slab_finish()
    slab.step_local(ranks)                                        # the contexts stay usable
    assert sum(s.live_count() for s in ranks) > 3000
    for s in ranks:
        s.close()
