"""Friends-of-friends groups on the device (psamd_groups / psamd_groups_result_get / psamd_download_groups, groups.hip) against
the numpy model (tests/groups_model.py), byte for byte: every output word is an integer that depends on the frame and the
radius alone, so there is no tolerance anywhere in this file.  `unfinished == 0` -- no union hit its step cap -- is part of
every comparison: the model's record says 0.

Frames.  Grids of 4^3 and 9^3 cells of 5 units.  The rough cloud is test_gpu_neighbours' (an empty cell, cells of 1, 63, 64, 65
and capacity + 6 particles, kids, an over-age particle, twins at one point, a pair across a cell wall) with forty small knots
added so that radius 0.4 finds groups of two and more (groups_model.rough_groups_cloud); the snake, the near-miss chains and
the dense clump are groups_model's.  tests/test_groups_cpu.py holds the model to a brute force on every one of these clouds and
asserts their shapes, so that nothing here can silently test an empty case."""
import ctypes as C

import numpy as np
import pytest
import torch

import groups_model as GM
import particlesystem_amd as ps
from particlesystem_amd import slab
from service_harness import DEV, ERR_INVALID_ARG, ERR_STATE, ERR_UNSUPPORTED, bits, captured, open_frame, same_state, slab_inputs
from test_gpu_neighbours import CS, GRIDS, QUIET, frame_of
from util import SENTINEL

pytestmark = pytest.mark.gpu

ARRAYS = ("group", "group_first", "group_size")
RECORD = ("members", "groups", "links", "singles", "largest", "unfinished")
ADULT = np.float32(3.0)


def context(G, cloud=None, flags=0, **over):
    """a context with the cloud filled -- xyz, all adults; none given: the rough cloud with its ages -- and the frame built;
    g.filled: the slot every row went to"""
    g = ps.ParticleSystem(ps.default_config(flags=flags, **{**GRIDS[G], **QUIET, **over}))
    xyz, age = GM.rough_groups_cloud(G, int(g.sizes.max_per_cell))
    if cloud is not None:
        xyz = xyz if isinstance(cloud, str) else cloud           # "rough": the rough cloud's places, no kids
        age = np.full(len(xyz), ADULT, np.float32)
    g.filled = np.asarray(g.fill_particles(xyz, age=age, fert_age=np.float32(1e6)), np.int64)
    assert (g.filled >= 0).all()
    open_frame(g)
    return g


def host_of(res):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


def same(got, want, what, keys=ARRAYS + RECORD):
    for k in keys:
        a, b = got[k], want[k]
        if k in RECORD:
            assert a == b, (what, k, a, b)
        else:
            assert a.dtype == b.dtype == np.int32 and np.array_equal(a, b), (what, k, a[:8], b[:8])


def raw_call(g, radius, live, room, flags=0, group=True):
    """psamd_groups through the spec, into buffers full of the sentinel: (group, group_first, group_size, the record)"""
    grp = torch.full((live + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    first = torch.full((room + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    size = torch.full((room + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    rec = torch.zeros(C.sizeof(ps.GroupsResult), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    spec = ps.GroupsSpec(flags=flags, radius=radius, group=grp.data_ptr() if group else None, capacity=live if group else 0,
                         group_first=first.data_ptr(), group_size=size.data_ptr(), group_capacity=room, result_dev=rec.data_ptr())
    assert g.lib.psamd_groups(g.h, C.byref(spec)) == 0
    g.synchronize()
    return grp.cpu().numpy(), first.cpu().numpy(), size.cpu().numpy(), ps.GroupsResult.from_device(rec).to_dict()


# ---- the rough cloud ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [4, 9])
def test_every_output_equals_the_model(G):
    g = context(G)
    fr = frame_of(g)
    assert g.counters["cell_overflow_kills"] == 6
    live = g.live_count()
    ids = g.export_live(ps.EXPORT_ID)["id"].cpu().numpy()
    full = None
    for radius in (CS, 0.4):
        want = GM.groups(fr, radius)
        got = host_of(g.groups(radius))
        print("G = %d, radius %g: %d members in %d groups (%d singles, largest %d), %d links, unfinished %d"
              % (G, radius, got["members"], got["groups"], got["singles"], got["largest"], got["links"], got["unfinished"]))
        assert np.array_equal(ids, want["ids"]) and len(got["group"]) == live and got["unfinished"] == 0
        same(got, want, "radius %g" % radius)
        assert got["links"] > 100 and (got["group"] == -1).any() and got["groups"] == len(got["group_size"])
        assert g.groups_result() == {k: got[k] for k in RECORD}
        # the host form is the same pass
        same(g.download_groups(radius), want, "host form, radius %g" % radius)
        # by export index: the same groups, group_first through the export's id array
        by = host_of(g.groups(radius, index=True))
        same(by, GM.groups(fr, radius, index=True), "index form, radius %g" % radius)
        assert np.array_equal(ids[by["group_first"]], got["group_first"]) and np.array_equal(by["group"], got["group"])
        full = got
    # (radius 0.4 from here on) tables too small: the prefix, the words past it untouched, group[] and the record unchanged
    record = {k: full[k] for k in RECORD}
    groups = full["groups"]
    assert groups > 30
    for room in (0, 1, groups - 1):
        grp, first, size, rec = raw_call(g, 0.4, live, room)
        assert np.array_equal(first[:room], full["group_first"][:room]) and (first[room:] == SENTINEL).all(), room
        assert np.array_equal(size[:room], full["group_size"][:room]) and (size[room:] == SENTINEL).all(), room
        assert np.array_equal(grp[:live], full["group"]) and (grp[live:] == SENTINEL).all() and rec == record, room
    # a capacity below the live count cuts group[] and nothing else
    for capacity in (live // 3, 1):
        short = host_of(g.groups(0.4, capacity=capacity))
        same(short, GM.groups(fr, 0.4, capacity=capacity), "capacity %d" % capacity)
        assert len(short["group"]) == capacity and np.array_equal(short["group_size"], full["group_size"])
    short = host_of(g.groups(0.4, index=True, capacity=live // 3))          # an index at or past the capacity is kept true
    same(short, GM.groups(fr, 0.4, capacity=live // 3, index=True), "index form under a capacity")
    assert (short["group_first"] >= live // 3).any()
    # no arrays at all: the record only
    _, first, size, rec = raw_call(g, 0.4, live, 0, group=False)
    assert rec == record and (first == SENTINEL).all()
    g.close()


def test_links_are_half_the_directed_pairs_on_a_cloud_without_kids():
    g = context(4, "rough")
    for radius in (0.4, CS):
        got = g.groups(radius)
        same(host_of(got), GM.groups(frame_of(g), radius), "no kids, radius %g" % radius)
        assert 2 * got["links"] == g.neighbours(radius, lists=False)["pairs"] > 0
        grp = got["group"]
        assert (grp >= 0).all() and torch.equal(torch.bincount(grp[grp >= 0].long()).int(), got["group_size"])
    g.close()


# ---- the snake: deep paths ------------------------------------------------------------------------------------------------------

def test_the_snake_is_one_group_whatever_slot_its_points_have():
    xyz, chain = GM.snake()
    g = context(4, xyz)
    n = len(xyz)
    slots = g.filled[chain]
    at = int(np.argmin(slots))
    assert 900 <= n <= 1200 and n // 10 < at < n - n // 10            # the root sits mid-chain: it has to travel both ways
    fr = frame_of(g)
    one = host_of(g.groups(0.4))
    same(one, GM.groups(fr, 0.4), "snake at 0.4")
    assert (one["groups"], one["largest"], one["links"], one["unfinished"]) == (1, n, n - 1, 0)
    assert one["group_first"][0] == slots.min() and (one["group"] == 0).all()
    apart = host_of(g.groups(0.29))
    same(apart, GM.groups(fr, 0.29), "snake at 0.29")
    assert (apart["groups"], apart["singles"], apart["links"], apart["unfinished"]) == (n, n, 0, 0)
    g.close()
    cut = 30
    xyz, chain = GM.snake(cut)
    g = context(4, xyz)
    two = host_of(g.groups(0.4))
    same(two, GM.groups(frame_of(g), 0.4), "broken snake")
    assert two["groups"] == 2 and sorted(two["group_size"].tolist()) == [cut, n - cut] and two["unfinished"] == 0
    ids = g.export_live(ps.EXPORT_ID)["id"].cpu().numpy()
    at = {int(i): k for k, i in enumerate(ids)}
    of = np.array([two["group"][at[int(s)]] for s in g.filled[chain]])
    assert len(set(of[:cut])) == 1 and len(set(of[cut:])) == 1 and of[0] != of[-1]
    g.close()


def test_one_ulp_of_d2_decides_a_link():
    xyz, radius = GM.near_miss()
    g = context(4, xyz)
    fr = frame_of(g)
    nxt = float(np.nextafter(np.float32(radius), np.float32(9)))
    apart, joined = host_of(g.groups(radius)), host_of(g.groups(nxt))
    same(apart, GM.groups(fr, radius), "near miss")
    same(joined, GM.groups(fr, nxt), "near miss, the next radius")
    assert (apart["groups"], apart["links"]) == (2, 8) and (joined["groups"], joined["links"], joined["largest"]) == (1, 9, 10)
    g.close()


def test_a_dense_clump_hooks_one_root_from_many_lanes():
    g = context(4, GM.clump(), max_particles_num=16384)
    got = host_of(g.groups(0.4))
    same(got, GM.groups(frame_of(g), 0.4), "clump")
    assert (got["groups"], got["largest"], got["links"], got["unfinished"]) == (1, 200, 200 * 199 // 2, 0)
    g.close()


# ---- graphs, state, force models ---------------------------------------------------------------------------------------------------

def test_a_graph_replays_the_plain_call_and_the_first_call_is_not_captured():
    g = context(9)
    live = g.live_count()
    rec = torch.zeros(C.sizeof(ps.GroupsResult), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    with captured(g) as cap:
        rc = g.lib.psamd_groups(g.h, C.byref(ps.GroupsSpec(radius=0.4, result_dev=rec.data_ptr())))       # the first call allocates the scratch
    assert rc == ERR_STATE
    cap.close()
    plain = host_of(g.groups(0.4))
    room = plain["groups"]
    bufs = dict(group=torch.full((live + 1,), SENTINEL, dtype=torch.int32, device=DEV),
                group_first=torch.full((room + 1,), SENTINEL, dtype=torch.int32, device=DEV),
                group_size=torch.full((room + 1,), SENTINEL, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    with captured(g) as cap:
        rc = g.lib.psamd_groups(g.h, C.byref(ps.GroupsSpec(radius=0.4, capacity=live, group_capacity=room, result_dev=rec.data_ptr(),
                                                           **{k: t.data_ptr() for k, t in bufs.items()})))
    assert rc == 0 and all((t == SENTINEL).all() for t in bufs.values())          # captured, not run
    cap.launch()
    got = {k: t.cpu().numpy()[:-1] for k, t in bufs.items()}
    got.update(ps.GroupsResult.from_device(rec).to_dict())
    same(got, plain, "graph replay")
    assert all(t.cpu().numpy()[-1] == SENTINEL for t in bufs.values())
    cap.close()
    same(host_of(g.groups(0.4)), plain, "the same call twice")
    g.calc_forces()
    g.synchronize()
    g.close()


def test_the_call_leaves_the_state_and_the_force_records_as_they_were():
    a, b = context(4), context(4)
    a.groups(CS)
    same_state(a, b, "after a call before the pair stage")
    a.calc_forces_pairs(); b.calc_forces_pairs()
    fa = a.download_force4(0, a.live_count())
    a.groups(0.4)
    assert np.array_equal(bits(a.download_force4(0, a.live_count())), bits(fa)), "the force records changed"
    same_state(a, b, "after a call behind the pair stage")
    a.calc_forces_apply(); b.calc_forces_apply()
    a.synchronize(); b.synchronize()
    same_state(a, b, "after the step")
    a.close(); b.close()


@pytest.mark.parametrize("flags", [ps.FLAG_FAR_PYRAMID, ps.FLAG_ALL_PAIRS, ps.FLAG_FAR_MONOPOLE, ps.FLAG_FAR_PYRAMID | ps.FLAG_FAR_QUADRUPOLE])
def test_the_groups_do_not_depend_on_the_force_model(flags):
    g, h = context(9), context(9, flags=flags)
    for radius in (CS, 0.4):
        same(host_of(h.groups(radius)), host_of(g.groups(radius)), "flags %#x, radius %g" % (flags, radius))
    g.close(); h.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable():
    g = ps.ParticleSystem(ps.default_config(**GRIDS[4], **QUIET))
    xyz, age = GM.rough_groups_cloud(4, int(g.sizes.max_per_cell))
    g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    n = len(xyz)
    buf = torch.zeros(n + 8, dtype=torch.int32, device=DEV)
    tab = torch.zeros(2 * (n + 8), dtype=torch.int32, device=DEV)
    rec = torch.zeros(64, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    good = dict(radius=0.4, group=buf.data_ptr(), capacity=n, group_first=tab.data_ptr(), group_size=tab.data_ptr() + 4 * (n + 8),
                group_capacity=n, result_dev=rec.data_ptr())

    def call(**kw):
        return g.lib.psamd_groups(g.h, C.byref(ps.GroupsSpec(**{**good, **kw})))
    assert call() == ERR_STATE                                   # no frame built
    g.init_iframe()
    assert call() == ERR_STATE
    g.build_grid()
    assert call() == 0
    for bad in (dict(flags=2), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")),
                dict(radius=float(np.nextafter(np.float32(CS), np.float32(9)))), dict(capacity=-1), dict(group_capacity=-1),
                dict(group=buf.data_ptr() + 2), dict(group_first=tab.data_ptr() + 1), dict(group_size=tab.data_ptr() + 2),
                dict(result_dev=rec.data_ptr() + 4)):
        assert call(**bad) == ERR_INVALID_ARG, bad
    assert call(radius=CS) == 0                                  # radius == cell_size is served
    assert g.lib.psamd_groups(g.h, None) == ERR_INVALID_ARG and g.lib.psamd_groups(None, C.byref(ps.GroupsSpec(**good))) == ERR_INVALID_ARG
    assert g.lib.psamd_groups_result_get(g.h, None) == ERR_INVALID_ARG
    assert call() == 0                                           # the refusals left the context usable
    g.synchronize()
    assert g.groups_result()["unfinished"] == 0 and g.groups_result()["groups"] > 30
    g.calc_forces()
    assert call() == ERR_STATE                                   # the frame has ended
    g.synchronize()
    g.close()


def test_a_slab_rank_is_refused_and_the_step_goes_on():
    xyz, age, v = slab_inputs(20000, 61)
    one = ps.ParticleSystem(ps.default_config())
    one.fill_particles(xyz, age=age, fert_age=np.float32(1e6), vxyz=v)
    ranks = [ps.ParticleSystem(ps.default_config(rank=r, world=2, cuts=[0, 7, 16])) for r in range(2)]
    plans = [s.slab_plan() for s in ranks]
    for s in ranks:
        s.fill_particles(xyz, age=age, fert_age=np.float32(1e6), vxyz=v)
    slab.to_pairs(ranks)
    for s in ranks:
        with pytest.raises(ps.PsamdError) as e:
            s.groups(0.4)
        assert e.value.status == ERR_UNSUPPORTED
        with pytest.raises(ps.PsamdError) as e:
            s.download_groups(0.4)
        assert e.value.status == ERR_UNSUPPORTED
        assert s.neighbours(0.4, lists=False)["pairs"] >= 0          # the context is usable: the window's other services run
    slab.apply_stage(ranks)
    slab.finish_stage(ranks)
    one.step(1)
    p = slab.merge_owned([s.download_particles() for s in ranks], plans)
    assert p.tobytes() == one.download_particles().tobytes(), "the step behind the refusal differs from the single context's"
    for s in ranks + [one]:
        s.synchronize()
        s.close()
