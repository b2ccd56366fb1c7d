"""Neighbour lists on the device (psamd_neighbours / psamd_neighbours_result_get / psamd_download_neighbours, neighbours.hip)
against the numpy model (tests/neighbours_model.py), byte for byte: every output word is an integer or one fp32 value with a
fixed operand order, so there is no tolerance anywhere in this file.

Frames.  Grids of 4^3 and 9^3 cells of 5 units (even and odd, both with box-face cells).  Among the cells of a frame are an
empty one, cells of 1, 63, 64 and 65 particles (the slice edge), and one that is given six more than MAX_PARTICLES_PER_CELL:
psamd_build_grid kills the surplus, as the reference does, so its list is full to the capacity and the surplus is in no export.
The count -1 -- a live particle that is in no list of the frame -- cannot be produced through the interface on one context
(every call that adds a particle ends the frame, which closes the window); the rule is the model's and is held there
(tests/test_neighbours_cpu.py).  The clouds also hold kids, an over-age particle, two particles at one
point and a pair straddling a cell wall.  With two particles at one point no radius lies below every pair distance: that
radius is checked on the same cloud without the second of the two.

Slabs: on the default 16^3 grid (chunk_dim 4) the group-aligned cuts, which lend nothing, fall at 3, 7 and 11
(tests/test_gpu_potential.py); a cut at 8 lends a layer and is the refusal case."""
import ctypes as C

import numpy as np
import pytest
import torch

import neighbours_model as M
import particlesystem_amd as ps
from particlesystem_amd import slab
from service_harness import DEV, ERR_INVALID_ARG, ERR_STATE, ERR_UNSUPPORTED, bits, captured, kid_age, open_frame, same_state, slab_inputs
from util import SENTINEL

pytestmark = pytest.mark.gpu

CS = 5.0
GRIDS = {4: dict(chunk_factor=1, chunk_dim=4, max_particles_num=4096), 9: dict(chunk_factor=3, chunk_dim=3, max_particles_num=65536)}
QUIET = dict(collision_radius=1e-6)            # nothing collides: the step that follows a call keeps every particle
SPECIAL = {"empty": (1, 2, 1), "one": (2, 1, 1), "n63": (1, 1, 2), "n64": (2, 2, 1), "n65": (1, 1, 1), "over": (2, 2, 2)}     # cells (i1, i2, i3)
ARRAYS = ("count", "nearest", "nearest_d2", "offsets", "list")
RECORD = ("listed", "pairs", "wanted", "max_count", "d2_min")


# ---- clouds -------------------------------------------------------------------------------------------------------------------

def in_cell(G, cell, frac):
    """xyz of points at the fractions frac [n, 3] of cell (i1, i2, i3): the cell axes are (-y, x, -z)"""
    q = -(G // 2) * CS + CS * (np.asarray(cell, np.float64)[None, :] + frac)
    return np.stack([q[:, 1], -q[:, 0], -q[:, 2]], 1).astype(np.float32)


def cell_of(G, xyz):
    q = np.stack([-xyz[:, 1], xyz[:, 0], -xyz[:, 2]], 1).astype(np.float64)
    i = np.floor(q / CS).astype(np.int64) + G // 2
    return (i[:, 2] * G + i[:, 0]) * G + i[:, 1]


def rough_cloud(G, cap, coincident=True, seed=5):
    """(xyz, age): a background of about six per cell with the special cells cleared, the special cells' own particles (tight
    enough for pairs within 0.4), every seventh a kid, one over age, two at one point, a pair across a cell wall"""
    rng = np.random.default_rng(seed + G)
    lo, hi = -(G // 2) * CS, (G - G // 2) * CS
    q = rng.uniform(lo + 0.001, hi - 0.001, (6 * G ** 3, 3))
    bg = np.stack([q[:, 1], -q[:, 0], -q[:, 2]], 1).astype(np.float32)
    special = {(c[2] * G + c[0]) * G + c[1] for c in SPECIAL.values()}
    bg = bg[~np.isin(cell_of(G, bg), list(special))]
    parts = [bg]
    for name, n in (("one", 1), ("n63", 63), ("n64", 64), ("n65", 65), ("over", cap + 6)):
        parts.append(in_cell(G, SPECIAL[name], rng.uniform(0.35, 0.65, (n, 3))))         # a 1.5-unit box: many pairs within 0.4
    wall = in_cell(G, (0, 1, 0), np.array([[0.5, 0.99, 0.5], [0.5, 1.01, 0.5]]))            # 0.1 apart, in two cells
    twin = in_cell(G, (0, 0, 1), np.array([[0.5, 0.5, 0.5]] * (2 if coincident else 1)))
    parts += [wall, twin]
    xyz = np.concatenate(parts).astype(np.float32)
    age = np.full(len(xyz), 3.0, np.float32)
    age[::7] = 0.5
    age[3] = 50.0                                   # over age (PARTICLE_LIFE is 15): a candidate like any other
    age[-4:] = 3.0                                  # the pair across the wall and the two at one point are adults
    return xyz, age


def context(G, coincident=True, flags=0, **over):
    g = ps.ParticleSystem(ps.default_config(flags=flags, **GRIDS[G], **QUIET, **over))
    cap = int(g.sizes.max_per_cell)
    assert g.sizes.grid_dim == G and cap >= 66, (g.sizes.grid_dim, cap)
    xyz, age = rough_cloud(G, cap, coincident)
    g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    open_frame(g)
    return g


# ---- the device against the model ----------------------------------------------------------------------------------------------

def frame_of(g, p=None, cg=None):
    p = g.download_particles() if p is None else p
    cg = g.download_cellgrid() if cg is None else cg
    return M.Frame(p, cg, g.sizes.grid_dim, kid_age(g.cfg), g.sizes.max_per_cell)


def host_of(res):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


def same(got, want, what, keys=ARRAYS + RECORD):
    for k in keys:
        a, b = got[k], want[k]
        if k in RECORD:
            assert a == b, (what, k, a, b)
        elif k == "nearest_d2":
            assert np.array_equal(bits(a), bits(b)), (what, k)
        else:
            assert a.dtype == b.dtype and np.array_equal(a, b), (what, k, a[:8], b[:8])


def shape_of(fr):
    """the frame has what the header of this file says"""
    G = fr.G
    n = {name: int(fr.count[(c[2] * G + c[0]) * G + c[1]]) for name, c in SPECIAL.items()}
    cap = fr.lists and max(len(l) for l in fr.lists)
    assert (n["empty"], n["one"], n["n63"], n["n64"], n["n65"]) == (0, 1, 63, 64, 65) and n["over"] == cap, n
    return cap


@pytest.mark.parametrize("G", [4, 9])
def test_every_output_equals_the_model(G):
    g = context(G)
    fr = frame_of(g)
    cap = shape_of(fr)
    assert g.counters["cell_overflow_kills"] == 6 and cap == g.sizes.max_per_cell
    live = g.live_count()
    ids = g.export_live(ps.EXPORT_ID)["id"].cpu().numpy()
    full = None
    for radius in (CS, 0.4):
        want = M.neighbours(fr, radius)
        got = host_of(g.neighbours(radius, nearest=True))
        print("G = %d, radius %g: %d queries, %d directed pairs, largest count %d, d2_min %g" % (G, radius, got["listed"], got["pairs"], got["max_count"], got["d2_min"]))
        assert np.array_equal(ids, want["ids"]) and got["listed"] == live == len(got["count"])
        same(got, want, "radius %g" % radius)
        assert got["pairs"] > 100 and got["d2_min"] == 0.0 and (got["count"] >= 0).all()
        assert g.neighbours_result() == {k: got[k] for k in RECORD}
        # the host form is the same pass
        same(g.download_neighbours(radius, nearest=True), want, "host form, radius %g" % radius)
        # by export index: the id lists mapped through the export's id array
        by = host_of(g.neighbours(radius, nearest=True, index=True))
        same(by, M.neighbours(fr, radius, index=True), "index form, radius %g" % radius)
        assert np.array_equal(ids[by["list"]], got["list"])
        full = got
    # (radius 0.4 from here on) a list too small: the prefix, the words past it untouched, `wanted` tells the truth
    wanted = full["wanted"]
    for room in (0, 1, wanted // 2, wanted - 1):
        out = torch.full((wanted + 8,), SENTINEL, dtype=torch.int32, device=DEV)
        offs = torch.zeros(live + 1, dtype=torch.int64, device=DEV)
        rec = torch.zeros(C.sizeof(ps.NeighboursResult), dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        spec = ps.NeighboursSpec(radius=0.4, offsets=offs.data_ptr(), capacity=live, list=out.data_ptr(), list_capacity=room, result_dev=rec.data_ptr())
        assert g.lib.psamd_neighbours(g.h, C.byref(spec)) == 0
        g.synchronize()
        a = out.cpu().numpy()
        assert np.array_equal(a[:room], full["list"][:room]) and (a[room:] == SENTINEL).all(), room
        assert ps.NeighboursResult.from_device(rec).to_dict() == {k: full[k] for k in RECORD} and np.array_equal(offs.cpu().numpy(), full["offsets"])
    # a capacity below the live count cuts the arrays and `wanted`, nothing else
    for capacity in (live // 3, 1):
        short = host_of(g.neighbours(0.4, nearest=True, capacity=capacity))
        same(short, M.neighbours(fr, 0.4, capacity=capacity), "capacity %d" % capacity)
        assert len(short["count"]) == capacity and short["wanted"] == full["offsets"][capacity] and short["pairs"] == full["pairs"]
    # capacity 0 without a list: the record only
    rec = torch.zeros(C.sizeof(ps.NeighboursResult), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    assert g.lib.psamd_neighbours(g.h, C.byref(ps.NeighboursSpec(radius=0.4, result_dev=rec.data_ptr()))) == 0
    g.synchronize()
    assert ps.NeighboursResult.from_device(rec).to_dict() == {**{k: full[k] for k in RECORD}, "wanted": 0}
    g.close()
    # a radius below every pair distance (the cloud without the second particle of the coincident pair)
    g = context(G, coincident=False)
    fr = frame_of(g)
    d2_min = M.neighbours(fr, CS)["d2_min"]
    assert d2_min > 0.0
    radius = float(np.float32(0.5 * np.sqrt(d2_min)))
    got = host_of(g.neighbours(radius, nearest=True))
    same(got, M.neighbours(fr, radius), "radius below every pair distance")
    assert (got["count"] == 0).all() and (got["nearest"] == -1).all() and np.isposinf(got["nearest_d2"]).all()
    assert got["pairs"] == got["wanted"] == got["max_count"] == 0 and got["d2_min"] == float("inf") and len(got["list"]) == 0
    g.close()


def test_a_graph_replays_the_plain_call_and_the_first_call_is_not_captured():
    g = context(9)
    live = g.live_count()
    bufs = dict(count=torch.full((live,), SENTINEL, dtype=torch.int32, device=DEV), nearest=torch.full((live,), SENTINEL, dtype=torch.int32, device=DEV),
                nearest_d2=torch.zeros(live, dtype=torch.float32, device=DEV), offsets=torch.zeros(live + 1, dtype=torch.int64, device=DEV))
    rec = torch.zeros(C.sizeof(ps.NeighboursResult), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    plain = None

    def spec_for(room, lst):
        return ps.NeighboursSpec(radius=0.4, capacity=live, list_capacity=room, result_dev=rec.data_ptr(), list=None if lst is None else lst.data_ptr(),
                                 **{k: t.data_ptr() for k, t in bufs.items()})
    with captured(g) as cap:
        rc = g.lib.psamd_neighbours(g.h, C.byref(spec_for(0, None)))            # the first call allocates the scratch
    assert rc == ERR_STATE
    cap.close()
    plain = host_of(g.neighbours(0.4, nearest=True))
    lst = torch.full((plain["wanted"] + 1,), SENTINEL, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    with captured(g) as cap:
        rc = g.lib.psamd_neighbours(g.h, C.byref(spec_for(plain["wanted"], lst)))
    assert rc == 0 and (lst == SENTINEL).all()                                   # captured, not run
    cap.launch()
    got = {k: t.cpu().numpy() for k, t in bufs.items()}
    got["list"] = lst.cpu().numpy()[:-1]
    got.update(ps.NeighboursResult.from_device(rec).to_dict())
    same(got, plain, "graph replay")
    assert lst.cpu().numpy()[-1] == SENTINEL
    cap.close()
    again = host_of(g.neighbours(0.4, nearest=True))
    same(again, plain, "the same call twice")
    g.calc_forces()
    g.synchronize()
    g.close()


def test_the_call_leaves_the_state_and_the_force_records_as_they_were():
    a, b = context(4), context(4)
    a.neighbours(CS, nearest=True)
    same_state(a, b, "after a call before the pair stage")
    a.calc_forces_pairs(); b.calc_forces_pairs()
    fa = a.download_force4(0, a.live_count())
    a.neighbours(0.4, nearest=True)
    assert np.array_equal(bits(a.download_force4(0, a.live_count())), bits(fa)), "the force records changed"
    same_state(a, b, "after a call behind the pair stage")
    a.calc_forces_apply(); b.calc_forces_apply()
    a.synchronize(); b.synchronize()
    same_state(a, b, "after the step")
    a.close(); b.close()


def test_refusals_leave_the_context_usable():
    g = ps.ParticleSystem(ps.default_config(**GRIDS[4], **QUIET))
    xyz, age = rough_cloud(4, int(g.sizes.max_per_cell))
    g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    n = len(xyz)
    buf = torch.zeros(n + 8, dtype=torch.int32, device=DEV)
    offs = torch.zeros(n + 8, dtype=torch.int64, device=DEV)
    rec = torch.zeros(64, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    good = dict(radius=0.4, count=buf.data_ptr(), offsets=offs.data_ptr(), capacity=n, result_dev=rec.data_ptr())

    def call(**kw):
        return g.lib.psamd_neighbours(g.h, C.byref(ps.NeighboursSpec(**{**good, **kw})))
    assert call() == ERR_STATE                                   # no frame built
    g.init_iframe()
    assert call() == ERR_STATE
    g.build_grid()
    assert call() == 0
    for bad in (dict(flags=2), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
                dict(radius=float(np.nextafter(np.float32(CS), np.float32(9)))), dict(capacity=-1), dict(list_capacity=-1),
                dict(count=buf.data_ptr() + 2), dict(nearest=buf.data_ptr() + 1), dict(nearest_d2=buf.data_ptr() + 2), dict(offsets=offs.data_ptr() + 4),
                dict(list=buf.data_ptr() + 2, list_capacity=4), dict(result_dev=rec.data_ptr() + 4), dict(list=buf.data_ptr(), list_capacity=4, offsets=None)):
        assert call(**bad) == ERR_INVALID_ARG, bad
    assert call(radius=CS) == 0                                  # radius == cell_size is served
    assert g.lib.psamd_neighbours(g.h, None) == ERR_INVALID_ARG and g.lib.psamd_neighbours(None, C.byref(ps.NeighboursSpec(**good))) == ERR_INVALID_ARG
    assert g.lib.psamd_neighbours_result_get(g.h, None) == ERR_INVALID_ARG
    assert call() == 0                                           # the refusals left the context usable
    g.calc_forces()
    assert call() == ERR_STATE                                   # the frame has ended
    g.synchronize()
    g.close()


@pytest.mark.parametrize("flags", [ps.FLAG_FAR_PYRAMID, ps.FLAG_ALL_PAIRS, ps.FLAG_FAR_MONOPOLE, ps.FLAG_FAR_PYRAMID | ps.FLAG_FAR_QUADRUPOLE])
def test_the_query_does_not_depend_on_the_force_model(flags):
    g, h = context(9), context(9, flags=flags)
    for radius in (CS, 0.4):
        same(host_of(h.neighbours(radius, nearest=True)), host_of(g.neighbours(radius, nearest=True)), "flags %#x, radius %g" % (flags, radius))
    g.close(); h.close()


# ---- slabs --------------------------------------------------------------------------------------------------------------------

def by_id(g, radius, container):
    """a context's outputs by global slot id: count (-2: not this context's), nearest, nearest_d2 bits, every particle's list"""
    res = host_of(g.neighbours(radius, nearest=True))
    ids = g.export_live(ps.EXPORT_ID)["id"].cpu().numpy()
    assert len(ids) == len(res["count"])
    count = np.full(container, -2, np.int32)
    near = np.full(container, -2, np.int32)
    d2 = np.zeros(container, np.uint32)
    count[ids], near[ids], d2[ids] = res["count"], res["nearest"], bits(res["nearest_d2"])
    assert np.array_equal(np.diff(res["offsets"]), np.maximum(res["count"], 0))
    lists = {int(i): res["list"][res["offsets"][k]:res["offsets"][k + 1]] for k, i in enumerate(ids)}
    return count, near, d2, lists, ids, res


@pytest.mark.parametrize("cuts,flags", [([0, 7, 16], 0), ([0, 3, 11, 16], 0), ([0, 7, 16], ps.FLAG_FAR_SLAB | ps.FLAG_FAR_PYRAMID),
                                        ([0, 3, 11, 16], ps.FLAG_FAR_SLAB | ps.FLAG_FAR_PYRAMID)])
def test_slabs_give_the_single_context_bytes(cuts, flags):
    xyz, age, v = slab_inputs(30000, 61)
    one = ps.ParticleSystem(ps.default_config(flags=flags & ~ps.FLAG_FAR_SLAB))
    one.fill_particles(xyz, age=age, fert_age=np.float32(1e6), vxyz=v)
    world = len(cuts) - 1
    ranks = [ps.ParticleSystem(ps.default_config(rank=r, world=world, cuts=cuts, flags=flags)) for r in range(world)]
    for s in ranks:
        s.fill_particles(xyz, age=age, fert_age=np.float32(1e6), vxyz=v)
    container = one.sizes.container_size
    for step in range(2):
        if step:
            one.step(1)
            slab.step_local(ranks)
        open_frame(one)
        slab.to_pairs(ranks)
        for radius in (CS, 0.4):
            count, near, d2, lists, ids, res = by_id(one, radius, container)
            if step == 0:
                same(res, M.neighbours(frame_of(one), radius), "the single context against the model, radius %g" % radius)
            u_count, u_near, u_d2, u_lists, parts, seen = np.full(container, -2, np.int32), np.full(container, -2, np.int32), np.zeros(container, np.uint32), {}, [], 0
            for s in ranks:
                pl = s.slab_plan()
                assert pl.lentin_lo == pl.lentin_hi and pl.lentout_lo == pl.lentout_hi
                c_r, n_r, d_r, l_r, ids_r, res_r = by_id(s, radius, container)
                assert (u_count[ids_r] == -2).all()
                u_count[ids_r], u_near[ids_r], u_d2[ids_r] = c_r[ids_r], n_r[ids_r], d_r[ids_r]
                u_lists.update(l_r)
                seen += len(ids_r)
                parts.append(res_r)
                with pytest.raises(ps.PsamdError) as e:
                    s.neighbours(radius, index=True)
                assert e.value.status == ERR_UNSUPPORTED
            what = "step %d, radius %g" % (step, radius)
            assert seen == len(ids) and np.array_equal(u_count, count) and np.array_equal(u_near, near) and np.array_equal(u_d2, d2), what
            assert u_lists.keys() == lists.keys() and all(np.array_equal(u_lists[i], lists[i]) for i in lists), what
            merged = ps.merge_neighbours(parts)
            assert merged == {k: res[k] for k in RECORD}, (what, merged)
            assert res["pairs"] > 0
        one.calc_forces()
        slab.apply_stage(ranks)
        slab.finish_stage(ranks)
    one.close()
    for s in ranks:
        s.close()


def test_a_lending_plan_and_an_all_pairs_world_are_refused_and_the_step_goes_on():
    xyz, age, v = slab_inputs(20000, 61)
    one = ps.ParticleSystem(ps.default_config())
    one.fill_particles(xyz, age=age, fert_age=np.float32(1e6), vxyz=v)
    ranks = [ps.ParticleSystem(ps.default_config(rank=r, world=2, cuts=[0, 8, 16])) for r in range(2)]
    plans = [s.slab_plan() for s in ranks]
    assert plans[0].lentout_lo < plans[0].lentout_hi and plans[1].lentin_lo < plans[1].lentin_hi
    for s in ranks:
        s.fill_particles(xyz, age=age, fert_age=np.float32(1e6), vxyz=v)
        with pytest.raises(ps.PsamdError) as e:
            s.neighbours(0.4)
        assert e.value.status == ERR_STATE                       # outside the window
    slab.to_pairs(ranks)
    for s in ranks:
        with pytest.raises(ps.PsamdError) as e:
            s.neighbours(0.4)
        assert e.value.status == ERR_UNSUPPORTED and "plan" in str(e.value)
    slab.apply_stage(ranks)
    slab.finish_stage(ranks)
    one.step(1)
    p = slab.merge_owned([s.download_particles() for s in ranks], plans)
    assert p.tobytes() == one.download_particles().tobytes(), "the step behind the refusal differs from the single context's"
    allp = [ps.ParticleSystem(ps.default_config(rank=r, world=2, cuts=[0, 7, 16], flags=ps.FLAG_ALL_PAIRS, max_particles_num=1 << 18)) for r in range(2)]
    for s in allp:
        s.fill_particles(xyz[:4000], age=age[:4000], fert_age=np.float32(1e6))
    slab.to_pairs(allp)
    for s in allp:
        with pytest.raises(ps.PsamdError) as e:
            s.neighbours(0.4)
        assert e.value.status == ERR_UNSUPPORTED
    slab.apply_stage(allp)
    slab.finish_stage(allp)
    for s in ranks + allp + [one]:
        s.synchronize()
        s.close()
