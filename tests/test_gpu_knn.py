"""The k nearest on the device (psamd_knn / psamd_knn_result_get / psamd_download_knn, knn.hip) against the numpy model
(tests/knn_model.py), byte for byte: every output word is an integer or one fp32 value with a fixed operand order -- d2 is
compared through bits() -- so there is no tolerance anywhere in this file.

Frames.  Grids of 4^3 and 9^3 cells of 5 units.  The rough frame is test_gpu_neighbours' (an empty cell, cells of 1, 63, 64, 65
and capacity + 6 particles, kids, an over-age particle, twins at one point, a pair across a cell wall); the tie lattices, the
lines and the one-ulp pair are knn_model's.  tests/test_knn_cpu.py holds the model to an fp64 ordering and asserts the clouds'
shapes, so that nothing here can silently test an empty case.  k runs over 1, 7, 8, 9 and 32: the kernel is instantiated for
rows of 1, 8, 16 and 32, so that is every tier, both sides of a tier edge and the maximum.

In ParticleSystem.knn's dict "found" is the array; the record's own `found`, the sum, stands under "found_sum"."""
import ctypes as C

import numpy as np
import pytest
import torch

import knn_model as KM
import particlesystem_amd as ps
from particlesystem_amd import slab
from service_harness import DEV, ERR_INVALID_ARG, ERR_STATE, ERR_UNSUPPORTED, bits, captured, open_frame, same_state, slab_inputs
from test_gpu_neighbours import CS, GRIDS, QUIET, context, frame_of, rough_cloud
from util import SENTINEL

pytestmark = pytest.mark.gpu

KS = (1, 7, 8, 9, 32)
ARRAYS = ("found", "who", "d2")
RECORD = KM.RECORD
ADULT = np.float32(3.0)
F_SENTINEL = np.float32(-77.0)


def host_of(res):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}


def same(got, want, what, keys=ARRAYS + RECORD):
    for k in keys:
        a, b = got[k], want[k]
        if k in RECORD:
            assert a == b, (what, k, a, b)
        elif k == "d2":
            assert a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(bits(a), bits(b)), (what, k)
        else:
            assert a.dtype == b.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), (what, k, a[:4], b[:4])


def record_of(res):
    """the record as psamd_knn_result_get has it"""
    return {("found" if k == "found_sum" else k): res[k] for k in RECORD}


def cloud_context(xyz, G=4, **over):
    """a context with the cloud filled, all adults, and the frame built; g.filled: the slot every row went to"""
    g = ps.ParticleSystem(ps.default_config(**{**GRIDS[G], **QUIET, **over}))
    g.filled = np.asarray(g.fill_particles(xyz, age=np.full(len(xyz), ADULT, np.float32), fert_age=np.float32(1e6)), np.int64)
    assert (g.filled >= 0).all()
    open_frame(g)
    return g


def raw_call(g, radius, k, rows, capacity, flags=0, arrays=True):
    """psamd_knn through the spec, into buffers of `rows` rows full of sentinels: (found, who, d2, the record)"""
    found = torch.full((rows + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    who = torch.full(((rows + 8) * k,), SENTINEL, dtype=torch.int32, device=DEV)
    d2 = torch.full(((rows + 8) * k,), float(F_SENTINEL), dtype=torch.float32, device=DEV)
    rec = torch.zeros(C.sizeof(ps.KnnResult), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    spec = ps.KnnSpec(flags=flags, radius=radius, k=k, capacity=capacity, result_dev=rec.data_ptr())
    if arrays:
        spec.found, spec.who, spec.d2 = found.data_ptr(), who.data_ptr(), d2.data_ptr()
    assert g.lib.psamd_knn(g.h, C.byref(spec)) == 0
    g.synchronize()
    return found.cpu().numpy(), who.cpu().numpy().reshape(-1, k), d2.cpu().numpy().reshape(-1, k), ps.KnnResult.from_device(rec).to_dict()


# ---- the rough frame ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [4, 9])
def test_every_output_equals_the_model(G):
    g = context(G)
    fr = frame_of(g)
    live = g.live_count()
    ids = g.export_live(ps.EXPORT_ID)["id"].cpu().numpy()
    for radius in (CS, 0.4):
        nb = host_of(g.neighbours(radius, lists=False, nearest=True))
        for k in KS:
            what = "G = %d, radius %g, k = %d" % (G, radius, k)
            want = KM.knn(fr, radius, k)
            got = host_of(g.knn(radius, k))
            print("%s: %d queries, found %d, full %d, dk2 in [%g, %g]" % (what, got["listed"], got["found_sum"], got["full"], got["dk2_min"], got["dk2_max"]))
            assert np.array_equal(ids, want["ids"]) and got["listed"] == live and got["who"].shape == (live, k)
            same(got, want, what)
            assert g.knn_result() == record_of(got), what
            assert np.array_equal(got["found"], np.minimum(nb["count"], k)), what        # (no count is -1 on one context)
            if k == 1:
                assert np.array_equal(got["who"][:, 0], nb["nearest"]) and np.array_equal(bits(got["d2"][:, 0]), bits(nb["nearest_d2"])), what
            # the host form is the same pass
            same(g.download_knn(radius, k), want, "host form, " + what)
            # by export index: the id rows mapped through the export's id array
            by = host_of(g.knn(radius, k, index=True))
            same(by, KM.knn(fr, radius, k, index=True), "index form, " + what)
            has = by["who"] >= 0
            assert np.array_equal(has, got["who"] >= 0) and np.array_equal(ids[by["who"][has]], got["who"][has]), what
        assert not host_of(g.knn(radius, 3, found=False)).keys() & {"found"}
    g.close()


@pytest.mark.parametrize("k", [7, 32])
def test_a_capacity_cuts_the_rows_and_nothing_else(k):
    g = context(9)
    fr = frame_of(g)
    live = g.live_count()
    whole = KM.knn(fr, 0.4, k)
    record = record_of(whole)
    for capacity in (live // 3, 1, 0):
        found, who, d2, rec = raw_call(g, 0.4, k, live, capacity)
        assert np.array_equal(found[:capacity], whole["found"][:capacity]) and (found[capacity:] == SENTINEL).all(), capacity
        assert np.array_equal(who[:capacity], whole["who"][:capacity]) and (who[capacity:] == SENTINEL).all(), capacity
        assert np.array_equal(bits(d2[:capacity]), bits(whole["d2"][:capacity])) and (d2[capacity:] == F_SENTINEL).all(), capacity
        assert rec == record, capacity
        short = host_of(g.knn(0.4, k, capacity=capacity))
        same(short, KM.knn(fr, 0.4, k, capacity=capacity), "capacity %d" % capacity)
        assert short["who"].shape == (capacity, k) and len(short["found"]) == capacity
        same(g.download_knn(0.4, k, capacity=capacity), short, "host form, capacity %d" % capacity)
    # an index at or past the capacity is kept true
    short = host_of(g.knn(0.4, k, index=True, capacity=live // 3))
    same(short, KM.knn(fr, 0.4, k, capacity=live // 3, index=True), "index form under a capacity")
    assert (short["who"] >= live // 3).any()
    # all three arrays NULL: result_dev alone
    found, who, d2, rec = raw_call(g, 0.4, k, live, live, arrays=False)
    assert rec == record and (found == SENTINEL).all() and (who == SENTINEL).all() and (d2 == F_SENTINEL).all()
    g.close()


# ---- the order ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("straddle", [False, True])
def test_ties_are_cut_inside_a_shell_by_the_lower_id(straddle):
    xyz, interior = KM.tie_lattice(straddle)
    g = cloud_context(xyz)
    fr = frame_of(g)
    slots = g.filled
    ids = g.export_live(ps.EXPORT_ID)["id"].cpu().numpy()
    at = {int(i): p for p, i in enumerate(ids)}
    r = xyz[:, None, :].astype(np.float64) - xyz[None, :, :]
    exact = (r * r).sum(2)
    for k, shell_d2, before in ((4, 1.0, 0), (8, 2.0, 6)):
        got = host_of(g.knn(1.5, k))
        same(got, KM.knn(fr, 1.5, k), "tie lattice, straddle %d, k = %d" % (straddle, k))
        for row in interior:
            p = at[int(slots[row])]
            shell = np.sort(slots[exact[row] == shell_d2])
            assert got["found"][p] == k and np.array_equal(got["who"][p, before:], shell[:k - before]) and (got["d2"][p, before:] == shell_d2).all(), (k, row)
    g.close()


@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("far_first", [True, False])
def test_arrival_orders(far_first, spread):
    xyz, query, near_to_far = KM.line(far_first, spread)
    g = cloud_context(xyz)
    got = host_of(g.knn(CS, 32))
    same(got, KM.knn(frame_of(g), CS, 32), "line, far first %d, spread %d" % (far_first, spread))
    ids = g.export_live(ps.EXPORT_ID)["id"].cpu().numpy()
    p = int(np.nonzero(ids == g.filled[query])[0][0])
    assert np.array_equal(got["who"][p], g.filled[near_to_far[:32]]) and (np.diff(got["d2"][p]) > 0).all() and got["found"][p] == 32
    if not spread:
        order = g.filled[near_to_far]
        assert (np.diff(order) < 0).all() if far_first else (np.diff(order) > 0).all()
    g.close()


@pytest.mark.parametrize("near_first", [True, False])
def test_one_ulp_of_d2_decides_the_order(near_first):
    xyz, query, near, far = KM.ulp_pair(near_first)
    g = cloud_context(xyz)
    fr = frame_of(g)
    ids = g.export_live(ps.EXPORT_ID)["id"].cpu().numpy()
    p = int(np.nonzero(ids == g.filled[query])[0][0])
    assert (g.filled[near] < g.filled[far]) == near_first
    for k in (1, 2, 9):
        got = host_of(g.knn(CS, k))
        same(got, KM.knn(fr, CS, k), "one ulp, k = %d" % k)
        assert got["who"][p, :2].tolist() == [g.filled[near], g.filled[far]][:k]
    a, b = got["d2"][p, :2]
    assert a == np.float32(0.5625) and b == np.nextafter(a, np.float32(1))
    g.close()


# ---- graphs, state, force models ---------------------------------------------------------------------------------------------------

def test_a_graph_replays_the_plain_call_and_the_first_call_is_not_captured():
    g = context(9)
    live = g.live_count()
    k = 9
    rec = torch.zeros(C.sizeof(ps.KnnResult), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    with captured(g) as cap:
        rc = g.lib.psamd_knn(g.h, C.byref(ps.KnnSpec(radius=0.4, k=k, result_dev=rec.data_ptr())))       # the first call allocates the scratch
    assert rc == ERR_STATE
    cap.close()
    plain = host_of(g.knn(0.4, k))
    bufs = dict(found=torch.full((live + 1,), SENTINEL, dtype=torch.int32, device=DEV),
                who=torch.full(((live + 1) * k,), SENTINEL, dtype=torch.int32, device=DEV),
                d2=torch.full(((live + 1) * k,), float(F_SENTINEL), dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    with captured(g) as cap:
        rc = g.lib.psamd_knn(g.h, C.byref(ps.KnnSpec(radius=0.4, k=k, capacity=live, result_dev=rec.data_ptr(), **{n: t.data_ptr() for n, t in bufs.items()})))
    assert rc == 0 and (bufs["found"] == SENTINEL).all() and (bufs["who"] == SENTINEL).all()          # captured, not run
    cap.launch()
    got = {"found": bufs["found"].cpu().numpy()[:-1], "who": bufs["who"].cpu().numpy().reshape(-1, k)[:-1], "d2": bufs["d2"].cpu().numpy().reshape(-1, k)[:-1]}
    r = ps.KnnResult.from_device(rec).to_dict()
    got.update({("found_sum" if n == "found" else n): v for n, v in r.items()})
    same(got, plain, "graph replay")
    assert bufs["found"].cpu().numpy()[-1] == SENTINEL and (bufs["who"].cpu().numpy().reshape(-1, k)[-1] == SENTINEL).all()
    cap.close()
    same(host_of(g.knn(0.4, k)), plain, "the same call twice")
    g.calc_forces()
    g.synchronize()
    g.close()


def test_the_call_leaves_the_state_and_the_force_records_as_they_were():
    a, b = context(4), context(4)
    a.knn(CS, 32)
    same_state(a, b, "after a call before the pair stage")
    a.calc_forces_pairs(); b.calc_forces_pairs()
    fa = a.download_force4(0, a.live_count())
    a.knn(0.4, 7)
    a.download_knn(CS, 1)
    assert np.array_equal(bits(a.download_force4(0, a.live_count())), bits(fa)), "the force records changed"
    same_state(a, b, "after a call behind the pair stage")
    a.calc_forces_apply(); b.calc_forces_apply()
    a.synchronize(); b.synchronize()
    same_state(a, b, "after the step")
    a.close(); b.close()


@pytest.mark.parametrize("flags", [ps.FLAG_FAR_PYRAMID, ps.FLAG_ALL_PAIRS, ps.FLAG_FAR_MONOPOLE, ps.FLAG_FAR_PYRAMID | ps.FLAG_FAR_QUADRUPOLE])
def test_the_rows_do_not_depend_on_the_force_model(flags):
    g, h = context(9), context(9, flags=flags)
    for radius, k in ((CS, 32), (0.4, 7)):
        same(host_of(h.knn(radius, k)), host_of(g.knn(radius, k)), "flags %#x, radius %g" % (flags, radius))
    g.close(); h.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable():
    g = ps.ParticleSystem(ps.default_config(**GRIDS[4], **QUIET))
    xyz, age = rough_cloud(4, int(g.sizes.max_per_cell))
    g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    n, k = len(xyz), 7
    buf = torch.zeros(n + 8, dtype=torch.int32, device=DEV)
    who = torch.zeros((n + 8) * k, dtype=torch.int32, device=DEV)
    d2 = torch.zeros((n + 8) * k, dtype=torch.float32, device=DEV)
    rec = torch.zeros(64, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    good = dict(radius=0.4, k=k, found=buf.data_ptr(), who=who.data_ptr(), d2=d2.data_ptr(), capacity=n, result_dev=rec.data_ptr())

    def call(**kw):
        return g.lib.psamd_knn(g.h, C.byref(ps.KnnSpec(**{**good, **kw})))
    assert call() == ERR_STATE                                   # no frame built
    g.init_iframe()
    assert call() == ERR_STATE
    g.build_grid()
    want = KM.knn(frame_of(g), 0.4, k)
    live = len(want["ids"])

    def good_call_equals_the_model(after):
        who.fill_(SENTINEL)
        torch.cuda.synchronize()
        assert call() == 0, after
        g.synchronize()
        got = {"found": buf.cpu().numpy()[:live], "who": who.cpu().numpy().reshape(-1, k)[:live], "d2": d2.cpu().numpy().reshape(-1, k)[:live]}
        same(got, want, after, ARRAYS)
        assert ps.KnnResult.from_device(rec[:C.sizeof(ps.KnnResult)]).to_dict() == record_of(want), after
    good_call_equals_the_model("the first call")
    for bad in (dict(k=0), dict(k=33), dict(k=-1), dict(reserved=1), dict(flags=2), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")),
                dict(radius=float("inf")), dict(radius=float(np.nextafter(np.float32(CS), np.float32(9)))), dict(capacity=-1),
                dict(capacity=1 << 60), dict(found=buf.data_ptr() + 2), dict(who=who.data_ptr() + 1), dict(d2=d2.data_ptr() + 2),
                dict(result_dev=rec.data_ptr() + 4)):
        assert call(**bad) == ERR_INVALID_ARG, bad
        good_call_equals_the_model(bad)
    assert call(radius=CS) == 0 and call(k=32, found=None, who=None, d2=None) == 0          # radius == cell_size and k == 32 are served
    assert g.lib.psamd_knn(g.h, None) == ERR_INVALID_ARG and g.lib.psamd_knn(None, C.byref(ps.KnnSpec(**good))) == ERR_INVALID_ARG
    assert g.lib.psamd_knn_result_get(g.h, None) == ERR_INVALID_ARG
    for bad in (dict(k=0), dict(k=33), dict(radius=0.0)):
        with pytest.raises(ps.PsamdError) as e:
            g.download_knn(**{**dict(radius=0.4, k=k), **bad})
        assert e.value.status == ERR_INVALID_ARG
    good_call_equals_the_model("the refusals")
    g.calc_forces()
    assert call() == ERR_STATE                                   # the frame has ended
    g.synchronize()
    g.close()


# ---- slabs --------------------------------------------------------------------------------------------------------------------

def by_id(g, radius, k, container):
    """a context's rows by global slot id: found (-2: not this context's), who, d2 bits"""
    res = host_of(g.knn(radius, k))
    ids = g.export_live(ps.EXPORT_ID)["id"].cpu().numpy()
    assert len(ids) == len(res["found"])
    found = np.full(container, -2, np.int32)
    who = np.full((container, k), -2, np.int32)
    d2 = np.zeros((container, k), np.uint32)
    found[ids], who[ids], d2[ids] = res["found"], res["who"], bits(res["d2"])
    return found, who, d2, ids, res


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
        for radius, k in ((CS, 9), (2.0, 2)):        # (30 000 in 80^3: about two neighbours within 2.0, full and short rows both)
            found, who, d2, ids, res = by_id(one, radius, k, container)
            if step == 0:
                same(res, KM.knn(frame_of(one), radius, k), "the single context against the model, radius %g" % radius)
            u_found, u_who, u_d2, parts, seen = np.full(container, -2, np.int32), np.full((container, k), -2, np.int32), np.zeros((container, k), np.uint32), [], 0
            for s in ranks:
                pl = s.slab_plan()
                assert pl.lentin_lo == pl.lentin_hi and pl.lentout_lo == pl.lentout_hi
                f_r, w_r, d_r, ids_r, res_r = by_id(s, radius, k, container)
                assert (u_found[ids_r] == -2).all()
                u_found[ids_r], u_who[ids_r], u_d2[ids_r] = f_r[ids_r], w_r[ids_r], d_r[ids_r]
                seen += len(ids_r)
                parts.append(res_r)
                with pytest.raises(ps.PsamdError) as e:
                    s.knn(radius, k, index=True)
                assert e.value.status == ERR_UNSUPPORTED
            what = "step %d, radius %g" % (step, radius)
            assert seen == len(ids) and np.array_equal(u_found, found) and np.array_equal(u_who, who) and np.array_equal(u_d2, d2), what
            merged = ps.merge_knn([record_of(r) for r in parts])
            assert merged == record_of(res), (what, merged)
            assert res["full"] > 0 and res["found_sum"] > res["full"]
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
            s.knn(0.4, 7)
        assert e.value.status == ERR_STATE                       # outside the window
    slab.to_pairs(ranks)
    for s in ranks:
        with pytest.raises(ps.PsamdError) as e:
            s.knn(0.4, 7)
        assert e.value.status == ERR_UNSUPPORTED and "plan" in str(e.value)
        with pytest.raises(ps.PsamdError) as e:
            s.download_knn(0.4, 7)
        assert e.value.status == ERR_UNSUPPORTED
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
            s.knn(0.4, 7)
        assert e.value.status == ERR_UNSUPPORTED
    slab.apply_stage(allp)
    slab.finish_stage(allp)
    for s in ranks + allp + [one]:
        s.synchronize()
        s.close()
