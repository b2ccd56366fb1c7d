"""A lattice field at the particles on the device (psamd_sample / psamd_sample_result_get, sample.hip).

What pins the arithmetic: the numpy model of tests/sample_model.py, written from include/psamd.h alone.  The order of an entry's
eight terms is fixed, so the device is held to the model BIT FOR BIT (a NaN compares as a NaN).  Everything else is byte
equality: the order form against the points form, twice, through a captured graph, mid-frame, every rank of a slab world
against one context; the adjointness with psamd_deposit within the bound tests/test_sample_cpu.py derives; and the loop the
service closes, deposit -> a field -> sample -> update's kick.  Shapes: 8^3 cells and the odd 9^3 (G / 2 rounds down), about
3 000 points; slabs on 16^3 with 8 000 particles."""
import ctypes as C

import numpy as np
import pytest
import torch

import deposit_model as D
import particlesystem_amd as ps
import sample_model as S
from particlesystem_amd import slab
from service_harness import DEV, ERR_INVALID_ARG, ERR_STATE, bits, captured, dev, open_frame, state
from util import SLOT_TILE, assert_same_particles, ragged

pytestmark = pytest.mark.gpu

CS = 5.0
GRIDS = {8: dict(max_particles_num=16384, chunk_factor=2, chunk_dim=4),      # the deposit test's shapes
         9: dict(max_particles_num=16384, chunk_factor=3, chunk_dim=3),      # G / 2 = 4: the box is not centred
         16: dict(max_particles_num=16384, chunk_factor=4, chunk_dim=4, x_factor=8)}
QUIET = dict(collision_radius=1e-6, drag=0.0)          # nothing collides
SENTINEL = 0x7fc0dead                                # what no sample writes


def points(G, seed=3):
    """about 3 000 points as pos4: uniform, on cell faces and one ulp either side, within h / 2 of every box face
    (sample_model.rough_points); exactly on voxel centres of every refine; outside the box; NaN, +-inf, 1e30"""
    rng = np.random.default_rng(seed + 50)
    xyz = [S.rough_points(G, CS, seed, n=(2000, 300, 300))]
    for k in D.REFINES:
        q = D.centres(G, CS, k).astype(np.float32)
        n = rng.integers(0, G * k, (80, 3))
        xyz.append(np.stack([q[n[:, 1]], -q[n[:, 0]], -q[n[:, 2]]], 1))
    half = G * CS
    out = rng.uniform(-half, half, (150, 3)).astype(np.float32)
    out[np.arange(150), rng.integers(0, 3, 150)] = np.where(np.arange(150) % 2 == 0, half + rng.uniform(0, 3, 150), -half - rng.uniform(0.001, 3, 150))
    odd = rng.uniform(-10, 10, (24, 3)).astype(np.float32)
    odd[np.arange(24), np.arange(24) % 3] = np.tile(np.array([np.nan, np.inf, -np.inf, 1e30], np.float32), 6)
    xyz += [out, odd]
    xyz = np.concatenate(xyz).astype(np.float32)
    xyz = xyz[rng.permutation(len(xyz))]
    return np.ascontiguousarray(np.concatenate([xyz, rng.uniform(1, 2, (len(xyz), 1)).astype(np.float32)], 1))


def lattice(G, refine, vec4, seed=7):
    """a random normal field with -0, a denormal and a few NaN / inf voxels planted"""
    M = G * refine
    rng = np.random.default_rng(seed + 10 * refine + G)
    F = rng.standard_normal((M, M, M, 4) if vec4 else (M, M, M)).astype(np.float32)
    flat = F.reshape(-1)
    at = rng.choice(flat.size, 40, replace=False)
    flat[at[:10]] = -0.0
    flat[at[10:20]] = np.float32(1e-41)
    flat[at[20:28]] = np.nan
    flat[at[28:34]] = np.inf
    flat[at[34:40]] = -np.inf
    return F


def same_words(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaNs differ at", np.nonzero(gn != wn)[0][:8])
    bad = (bits(got) != bits(want)) & ~wn
    assert not bad.any(), (what, "words differ at", np.argwhere(bad)[:8], got[bad][:4], want[bad][:4])


@pytest.fixture(scope="module")
def bare():
    """per grid one context that has never built a grid: the points form reads no frame"""
    made = {}

    def get(G):
        if G not in made:
            made[G] = ps.ParticleSystem(ps.default_config(**GRIDS[G], **QUIET))
            assert made[G].sizes.grid_dim == G
        return made[G]
    yield get
    for g in made.values():
        g.close()


@pytest.fixture(scope="module")
def pts():
    return {G: points(G) for G in (8, 9, 16)}


# ---- 1. the device against the model, bit for bit ------------------------------------------------------------------------------

@pytest.mark.parametrize("vec4", [False, True])
@pytest.mark.parametrize("refine", D.REFINES)
@pytest.mark.parametrize("G", [8, 9])
def test_device_against_the_model(bare, pts, G, refine, vec4):
    g, pos4 = bare(G), pts[G]
    m, n = len(pos4), len(pos4) - 137
    F = lattice(G, refine, vec4)
    want, w_oc, w_res, _ = S.sample(pos4[:n, 0], pos4[:n, 1], pos4[:n, 2], F, G, CS, scale=1.75)
    assert w_res["outside"] > 150 and w_res["nonfinite"] > 0 and w_res["served"] > 2500
    out = torch.from_numpy(np.full((m, 4) if vec4 else (m,), SENTINEL, np.uint32).view(np.float32)).to(DEV)
    count = torch.full((1,), n, dtype=torch.int64, device=DEV)
    got, oc, res = g.sample(dev(F), pos4=dev(pos4), count=count, scale=1.75, out=out, outcome=True, result=True)
    got, oc = got.cpu().numpy(), oc.cpu().numpy()
    same_words(got[:n], want, "%d^3 refine %d vec4 %s" % (G, refine, vec4))
    assert (bits(got[:n][w_oc == 1]) == S.QNAN).all(), "an outside entry's words are not the quiet NaN 0x7fc00000"
    assert (bits(got[n:]) == SENTINEL).all(), "entries at or past n were touched"
    assert np.array_equal(oc[:n], w_oc) and (oc[n:] == -1).all()
    assert res == w_res and g.sample_result() == res
    # no count: all m entries, and a fresh out
    got2, res2 = g.sample(dev(F), pos4=dev(pos4), scale=1.75, result=True)
    want2, _, w_res2, _ = S.sample(pos4[:, 0], pos4[:, 1], pos4[:, 2], F, G, CS, scale=1.75)
    same_words(got2.cpu().numpy(), want2, "no count")
    assert res2 == w_res2 and res2["done"] == m


# ---- 2. export order equals the points form ------------------------------------------------------------------------------------

def test_export_order_equals_the_points_form():
    """18 000 owned slots: four slot tiles and one of 1616; holes from a removal and from the steps' deaths"""
    g, rec = ragged(seed=37)
    g.remove(ids=dev(rec["id"][::3].astype(np.int32)))
    g.step(3)
    p = g.download_particles()
    # (an upload files a coordinate that is no number under one fixed index of its axis: on 8^3 cells index 0 -- x is axis i2)
    assert g.sizes.grid_dim == 8
    live_ids = np.nonzero((p["cell"] >= 0) & (p["cell"] < g.sizes.num_cells) & (p["cell"] % 8 == 0))[0]
    b = int(live_ids[len(live_ids) // 2])
    p["x"][b] = np.nan
    g.upload_particles(p[b:b + 1], first=b)
    G, cs = g.sizes.grid_dim, float(g.cfg.cell_size)
    ex = g.export_live(ps.EXPORT_POS | ps.EXPORT_ID)
    live, eid = ex["count"], ex["id"].cpu().numpy()
    assert 1000 < live < len(rec) - len(rec[::3]) + 1 and len(set(eid // SLOT_TILE)) > 2 and g.owned_slots() > 4 * SLOT_TILE
    kb = int(np.nonzero(eid == b)[0][0])
    for vec4 in (False, True):
        rng = np.random.default_rng(5)
        F = dev(rng.standard_normal((2 * G,) * 3 + ((4,) if vec4 else ())).astype(np.float32))
        a, a_oc, a_res = g.sample(F, outcome=True, result=True)
        c, c_oc, c_res = g.sample(F, pos4=ex["pos4"], outcome=True, result=True)
        assert a.shape[0] == g.owned_slots() and c.shape[0] == live
        assert bits(a[:live]).tobytes() == bits(c).tobytes(), "export order differs from the points form"
        assert (bits(a[live:]) == 0).all() and (a_oc[live:] == -1).all().item(), "entries at or past the live count were touched"
        assert np.array_equal(a_oc[:live].cpu().numpy(), c_oc.cpu().numpy()) and a_res == c_res and a_res["done"] == live
        assert int(a_oc[kb]) == 1 and a_res["outside"] >= 1 and (bits(a[kb]) == S.QNAN).all(), "a live particle with a NaN x"
        # ... and the model, at the export's positions
        pos = ex["pos4"].cpu().numpy()
        want, w_oc, w_res, _ = S.sample(pos[:, 0], pos[:, 1], pos[:, 2], F.cpu().numpy(), G, cs)
        same_words(c.cpu().numpy(), want, "the points form at the export's positions")
        assert w_res == c_res
        # fewer entries than live particles: the particles past n are not served
        n = live - 777
        out = torch.from_numpy(np.full((live, 4) if vec4 else (live,), SENTINEL, np.uint32).view(np.float32)).to(DEV)
        count = torch.full((1,), n, dtype=torch.int64, device=DEV)
        d, d_res = g.sample(F, count=count, out=out, result=True)
        assert bits(d[:n]).tobytes() == bits(c[:n]).tobytes() and (bits(d[n:]) == SENTINEL).all() and d_res["done"] == n
    g.close()


# ---- 3. the same bytes twice, through a captured graph, mid-frame ----------------------------------------------------------------

def stepped(steps=3):
    rng = np.random.default_rng(11)
    n = 4000
    g = ps.ParticleSystem(ps.default_config(**GRIDS[8]))
    xyz = rng.uniform(-19.9, 19.9, (n, 3)).astype(np.float32)
    g.fill_particles(xyz, age=rng.uniform(0.2, 9.0, n).astype(np.float32), fert_age=np.float32(1e6),
                     vxyz=rng.uniform(-8, 8, (n, 3)).astype(np.float32))
    g.step(steps)
    return g


def state_of(g):
    return [a.tobytes() for a in state(g)]


@pytest.mark.parametrize("vec4", [False, True])
def test_same_bytes_twice_through_a_graph_and_mid_frame(pts, vec4):
    g, h = stepped(), stepped()
    pos4 = dev(pts[8])
    m, slots = len(pts[8]), g.owned_slots()
    F = dev(lattice(8, 2, vec4))
    before = state_of(g)
    a, ra = g.sample(F, pos4=pos4, result=True)                    # between frames
    o, ro = g.sample(F, result=True)
    assert state_of(g) == before, "the samples touched particles or queues"
    open_frame(g)
    open_frame(h)
    a2, ra2 = g.sample(F, pos4=pos4, result=True)
    o2, ro2 = g.sample(F, result=True)
    assert bits(a).tobytes() == bits(a2).tobytes() and ra == ra2 and bits(o).tobytes() == bits(o2).tobytes() and ro == ro2
    assert ro["done"] == g.live_count() > 3000
    # captured into a caller's graph (the call allocates nothing) and replayed, both forms
    shape = lambda k: (k, 4) if vec4 else (k,)
    ga = torch.full(shape(m), float("nan"), dtype=torch.float32, device=DEV)
    go = torch.zeros(shape(slots), dtype=torch.float32, device=DEV)
    rec = torch.zeros(2 * C.sizeof(ps.SampleResult), dtype=torch.uint8, device=DEV)
    common = dict(refine=2, field=F.data_ptr(), capacity=16 ** 3, scale=1.0)
    sa = ps.SampleSpec(flags=int(vec4), pos4=pos4.data_ptr(), max_count=m, out=ga.data_ptr(), result_dev=rec.data_ptr(), **common)
    so = ps.SampleSpec(flags=int(vec4) | ps.SAMPLE_EXPORT_ORDER, max_count=slots, out=go.data_ptr(), result_dev=rec.data_ptr() + 32, **common)
    with captured(g) as cap:
        rcs = [g.lib.psamd_sample(g.h, C.byref(sa)), g.lib.psamd_sample(g.h, C.byref(so))]
    assert rcs == [0, 0]
    cap.launch()
    assert bits(ga).tobytes() == bits(a).tobytes() and bits(go).tobytes() == bits(o).tobytes()
    assert ps.SampleResult.from_device(rec[:32]).to_dict() == ra and ps.SampleResult.from_device(rec[32:]).to_dict() == ro
    cap.close()
    # between the pair stage and the apply stage
    g.calc_forces_pairs()
    h.calc_forces_pairs()
    before = state_of(g)
    a3, ra3 = g.sample(F, pos4=pos4, result=True)
    o3, ro3 = g.sample(F, result=True)
    assert bits(a3).tobytes() == bits(a).tobytes() and ra3 == ra and bits(o3).tobytes() == bits(o).tobytes() and ro3 == ro
    assert state_of(g) == before, "the samples touched particles or queues mid-frame"
    g.calc_forces_apply()
    h.calc_forces_apply()
    g.step(1)
    h.step(1)
    assert state_of(g) == state_of(h), "the steps after the samples differ from a run without them"
    g.close(); h.close()


# ---- 4. slabs --------------------------------------------------------------------------------------------------------------------

def slab_cloud(G, n, seed=61):
    rng = np.random.default_rng(seed)
    half = G * 2.5 * 0.9995
    return dict(xyz=rng.uniform(-half, half, (n, 3)).astype(np.float32), age=rng.uniform(0.2, 9.0, n).astype(np.float32),
                w=rng.uniform(20.0, 100.0, n).astype(np.float32), fert_age=np.float32(1e6), vxyz=rng.uniform(-8, 8, (n, 3)).astype(np.float32))


def ranks_against_one(one, ranks, G, pos4, vec4):
    """every rank, given all points, returns the single context's bytes; by export order a rank's output pairs with its own
    export and the union, by id, is the single context's"""
    F = dev(lattice(G, 2, vec4))
    want, w_oc, w_res = one.sample(F, pos4=pos4, outcome=True, result=True)
    ex1 = one.export_live(ps.EXPORT_ID)
    o1 = one.sample(F)
    by_id = {}
    recs = []
    for s in ranks:
        got, oc, res = s.sample(F, pos4=pos4, outcome=True, result=True)
        assert bits(got).tobytes() == bits(want).tobytes() and torch.equal(oc, w_oc) and res == w_res
        ex = s.export_live(ps.EXPORT_ID | ps.EXPORT_POS)
        o, ores = s.sample(F, result=True)
        k = ex["count"]
        assert o.shape[0] == s.owned_slots() and ores["done"] == k and (bits(o[k:]) == 0).all()
        assert bits(o[:k]).tobytes() == bits(s.sample(F, pos4=ex["pos4"])).tobytes()
        recs.append(ores)
        for i, row in zip(ex["id"].cpu().numpy().tolist(), bits(o[:k]).reshape(k, -1)):
            assert i not in by_id
            by_id[i] = row.tobytes()
    ids1 = ex1["id"].cpu().numpy().tolist()
    assert sorted(by_id) == ids1 and len(ids1) > 2000
    assert all(by_id[i] == row.tobytes() for i, row in zip(ids1, bits(o1[:len(ids1)]).reshape(len(ids1), -1)))
    assert ps.merge_sample(recs) == one.sample_result()


@pytest.mark.parametrize("world,cuts", [(2, [0, 8, 16]), (2, [0, 7, 16]), (3, None)])
def test_slabs_give_the_single_context_bytes(pts, world, cuts):
    inputs = slab_cloud(16, 8000)
    over = dict(GRIDS[16], **({"cuts": cuts} if cuts else {}))
    one = ps.ParticleSystem(ps.default_config(**GRIDS[16]))
    one.fill_particles(**inputs)
    ranks = [ps.ParticleSystem(ps.default_config(rank=r, world=world, **over)) for r in range(world)]
    for s in ranks:
        s.fill_particles(**inputs)
    one.step(1)
    slab.step_local(ranks)
    pos4 = dev(pts[16])
    ranks_against_one(one, ranks, 16, pos4, False)                # between frames
    open_frame(one)
    slab.to_pairs(ranks)
    ranks_against_one(one, ranks, 16, pos4, True)                 # mid-frame
    one.calc_forces()
    slab.apply_stage(ranks)
    slab.finish_stage(ranks)
    assert sum(s.live_count() for s in ranks) == one.live_count() > 7000       # the steps went on
    one.close()
    for s in ranks:
        s.close()


def test_a_far_slab_is_served(pts):
    inputs = slab_cloud(8, 3000, seed=62)
    flags = ps.FLAG_FAR_PYRAMID
    one = ps.ParticleSystem(ps.default_config(flags=flags, **GRIDS[8]))
    one.fill_particles(**inputs)
    ranks = [ps.ParticleSystem(ps.default_config(flags=flags | ps.FLAG_FAR_SLAB, rank=r, world=2, **GRIDS[8])) for r in range(2)]
    for s in ranks:
        s.fill_particles(**inputs)
    open_frame(one)
    slab.to_pairs(ranks)
    ranks_against_one(one, ranks, 8, dev(pts[8]), True)
    one.calc_forces()
    slab.apply_stage(ranks)
    slab.finish_stage(ranks)
    slab.step_local(ranks)
    assert sum(s.live_count() for s in ranks) > 2000
    one.synchronize()
    one.close()
    for s in ranks:
        s.close()


# ---- 5. adjointness on the device -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("refine", D.REFINES)
@pytest.mark.parametrize("G", [8, 9])
def test_the_device_sample_is_the_adjoint_of_the_device_deposit(G, refine):
    """no list overflow, no kids, finite bodies: the deposit's bodies are the export's particles with m = |w|"""
    xyz = S.rough_points(G, CS, 3)
    rng = np.random.default_rng(103)
    w = rng.uniform(20.0, 100.0, len(xyz)).astype(np.float32)
    w[::29] = 0.0
    g = ps.ParticleSystem(ps.default_config(**GRIDS[G], **QUIET))
    g.fill_particles(xyz, age=np.full(len(xyz), 3.0, np.float32), w=w, fert_age=np.float32(1e6))
    open_frame(g)
    rho, dres = g.deposit(refine, result=True)
    ex = g.export_live(ps.EXPORT_POS)
    pos = ex["pos4"].cpu().numpy()
    assert dres["bodies"] == ex["count"] == len(xyz) and dres["skipped"] == 0 and g.counters["cell_overflow_kills"] == 0
    M = G * refine
    F = rng.standard_normal((M, M, M)).astype(np.float32)
    smp, res = g.sample(dev(F), result=True)
    assert res["served"] == len(xyz)
    _, _, _, Sk = S.sample(pos[:, 0], pos[:, 1], pos[:, 2], F, G, CS)
    err, scale = S.adjoint_sides(F, rho.cpu().numpy(), np.abs(pos[:, 3]), smp[:len(xyz)].cpu().numpy(), Sk)
    print("%d^3 cells, refine %d: |sum F rho - sum m sample| / (2^-24 sum m S) = %.3g" % (G, refine, err / (2.0 ** -24 * scale)))
    assert err <= 5.0 * 2.0 ** -24 * scale
    g.close()


# ---- 6. the kick loop ---------------------------------------------------------------------------------------------------------------

def test_the_kick_loop():
    g = stepped()
    open_frame(g)
    rho = g.deposit(2)
    smooth = sum(torch.roll(rho, s, a) for a in range(3) for s in (-1, 1)) / 6.0 + rho
    grad = [torch.roll(smooth, -1, a) - torch.roll(smooth, 1, a) for a in (2, 1, 0)]      # along n2, n1, n3: x, -y, -z
    field4 = torch.stack([-grad[0], grad[1], grad[2], smooth], 3).contiguous() * 1e-3
    dt = 0.01
    p0, qi0, q0 = state(g)
    ids = g.export_live(ps.EXPORT_ID)["id"].cpu().numpy()
    dv = g.sample(field4, scale=dt)
    r = g.update(vel4=dv, add=True)
    assert r["updated"] == len(ids) > 3000 and r["not_live"] == g.owned_slots() - len(ids)
    p1, qi1, q1 = state(g)
    d = dv[:len(ids)].cpu().numpy()
    assert np.isfinite(d).all() and (d[:, :3] != 0).any(1).sum() > 3000
    want = np.frombuffer(bytearray(p0.tobytes()), p0.dtype)         # (a copy of a record array leaves its pad bytes undefined)
    for k, name in enumerate(("vx", "vy", "vz")):
        want[name][ids] = p0[name][ids].astype(np.float32) + d[:, k].astype(np.float32)
    assert_same_particles(p1, want, "the velocities after the kick")
    assert qi1.tobytes() == qi0.tobytes() and q1.tobytes() == q0.tobytes()
    g.calc_forces()                                               # the frame goes on
    g.step(1)
    g.synchronize()
    g.close()


# ---- 7. arguments and refusals ----------------------------------------------------------------------------------------------------

def test_arguments(bare):
    g = bare(8)
    M3, m = 16 ** 3, 100
    F = torch.zeros((M3 + 1) * 4, dtype=torch.float32, device=DEV)
    pos = torch.zeros((m + 1) * 4, dtype=torch.float32, device=DEV)
    out = torch.zeros((m + 1) * 4, dtype=torch.float32, device=DEV)
    oc = torch.zeros(m + 1, dtype=torch.int32, device=DEV)
    cnt = torch.full((2,), m, dtype=torch.int64, device=DEV)
    rec = torch.zeros(64, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    good = dict(flags=ps.SAMPLE_VEC4, refine=2, field=F.data_ptr(), capacity=M3, pos4=pos.data_ptr(), max_count=m, count_dev=cnt.data_ptr(),
                out=out.data_ptr(), scale=1.0, reserved=0, outcome_dev=oc.data_ptr(), result_dev=rec.data_ptr())

    def call(**kw):
        with g._on_stream(DEV):
            return g.lib.psamd_sample(g.h, C.byref(ps.SampleSpec(**{**good, **kw})))
    assert call() == 0 and g.sample_result() == dict(done=m, served=m, outside=0, nonfinite=0)
    order = ps.SAMPLE_EXPORT_ORDER
    for bad in (dict(flags=4), dict(flags=ps.SAMPLE_VEC4 | 0x80000000), dict(reserved=1), dict(refine=0), dict(refine=3), dict(refine=8),
                dict(refine=-1), dict(capacity=M3 - 1), dict(refine=4), dict(max_count=-1), dict(max_count=2 ** 31), dict(field=None),
                dict(out=None), dict(pos4=None), dict(flags=order, pos4=pos.data_ptr()), dict(pos4=pos.data_ptr() + 4),
                dict(field=F.data_ptr() + 4), dict(out=out.data_ptr() + 8), dict(flags=0, field=F.data_ptr() + 2),
                dict(flags=0, out=out.data_ptr() + 1), dict(outcome_dev=oc.data_ptr() + 2), dict(count_dev=cnt.data_ptr() + 4),
                dict(result_dev=rec.data_ptr() + 4)):
        assert call(**bad) == ERR_INVALID_ARG, bad
        assert b"sample" in g.lib.psamd_last_error(g.h)
    assert g.lib.psamd_sample(g.h, None) == ERR_INVALID_ARG and g.lib.psamd_sample_result_get(g.h, None) == ERR_INVALID_ARG
    # what is valid: a float lattice on 4 bytes, the order form without pos4, every optional pointer left out
    assert call(flags=0, field=F.data_ptr() + 4, out=out.data_ptr() + 4) == 0
    assert call(flags=order, pos4=None) == 0 and g.sample_result()["done"] == 0            # (the context holds no particle)
    assert call(count_dev=None, outcome_dev=None, result_dev=None) == 0 and g.sample_result()["done"] == m
    assert ps.SampleResult.from_device(rec[:32]).to_dict() == dict(done=0, served=0, outside=0, nonfinite=0)     # the order form's
    # max_count == 0 writes a zero record, with nothing else given
    assert call(max_count=0, pos4=None, out=None) == 0
    assert g.sample_result() == dict(done=0, served=0, outside=0, nonfinite=0)
    assert call() == 0 and ps.SampleResult.from_device(rec[:32]).to_dict() == g.sample_result() == dict(done=m, served=m, outside=0, nonfinite=0)


def test_export_order_is_refused_between_slab_apply_and_slab_finish(pts):
    inputs = slab_cloud(8, 3000, seed=63)
    ranks = [ps.ParticleSystem(ps.default_config(rank=r, world=2, **GRIDS[8])) for r in range(2)]
    for s in ranks:
        s.fill_particles(**inputs)
    F = dev(lattice(8, 1, False))
    pos4 = dev(pts[8])
    want = ranks[0].sample(F, pos4=pos4)
    seen = []

    def refused(rs):
        for s in rs:
            with pytest.raises(ps.PsamdError) as e:
                s.sample(F)
            assert e.value.status == ERR_STATE and b"slab_apply" in s.lib.psamd_last_error(s.h)
            seen.append(bits(s.sample(F, pos4=pos4)).tobytes())        # the points form is served all the same
    torch.cuda.synchronize()
    slab.step_local(ranks, after_apply=refused)
    assert seen == [bits(want).tobytes()] * 2
    slab.step_local(ranks)                                             # the contexts stay usable
    live = sum(s.live_count() for s in ranks)
    assert live > 2000 and sum(s.sample(F, result=True)[1]["done"] for s in ranks) == live
    for s in ranks:
        s.close()
