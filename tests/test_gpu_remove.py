"""Taking particles out (psamd_remove / psamd_remove_result_get, remove.hip): the device-side, stream-ordered kill.  What
must hold: after a remove, the particle arrays, the queues and their records, the outcomes and the result record are
byte-equal to what the oracle's serial get_id_info + reset_particle + q_insert leave over the same candidates in the same
order (tests/remove_model.py: serial) -- by id and by box, with graphs on and off, run-ahead 0 and 1, at the corners of
q_insert (an emptied record, a rear about to wrap, a full record), with a device-written count, on slabs -- and the steps,
injects and snapshots that follow see a usable state."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import particlesystem_amd as ps
import remove_model as M
from particlesystem_amd.slab import merge_owned, step_local
from service_harness import DEV, ERR_INVALID_ARG, ERR_STATE, OK, batch, captured, dev, inject, many_records, same_state, start, state
from util import SLOT_TILE, assert_same_particles, cloud, ragged

pytestmark = pytest.mark.gpu

TILE = 4096          # inject's and remove's tile of entries


def remove_ids(g, ids, count=None):
    r = g.remove(ids=dev(np.asarray(ids, np.int32)), count=count, outcome=True)
    out = r.pop("outcome").cpu().numpy()
    return r, out


def same_as_oracle(g, o, what):
    p, qi, q = state(g)
    assert_same_particles(p, o.particles, what + ": particles")
    assert qi.tobytes() == o.queue_info.tobytes(), what + ": QUEUE_INFO records differ"
    assert np.array_equal(q, o.queue), what + ": queues differ"


def check_by_id(g, o, ids, what, count=None, n=None):
    """remove on the GPU, the serial definition on the oracle over the first n entries: everything equal"""
    n = len(ids) if n is None else n
    r, out = remove_ids(g, ids, count)
    s_out, s_res = M.serial(o, ids[:n])
    assert np.array_equal(out[:n], s_out), (what, np.nonzero(out[:n] != s_out)[0][:10])
    assert (out[n:] == -1).all(), what + ": outcomes past n"
    assert r == s_res, (what, r, s_res)
    assert g.remove_result() == r
    same_as_oracle(g, o, what)
    return r, out


def mixed_ids(g, o, rng):
    """at least two tiles: live ids, free slots, invalid ids, duplicates inside a 64-entry group, across the waves of a
    tile and across tiles, and the slots of the fullest records in descending order"""
    cont = g.sizes.container_size
    p, qi = o.particles, o.queue_info
    live = np.nonzero(p["cell"] >= 0)[0]
    free = np.nonzero(p["cell"] < 0)[0]
    ids = np.concatenate([rng.choice(live, 5000), rng.choice(free, 1500), rng.integers(-1000, 0, 60),
                          rng.integers(cont, cont + 1000, 60), [np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1, cont]])
    rng.shuffle(ids)
    lo = qi["rloc"].astype(np.int64)
    per_rec = np.array([(p["cell"][a:a + s] >= 0).sum() for a, s in zip(lo, qi["seg_size"])])
    runs = [np.arange(lo[r] + qi["seg_size"][r] - 1, lo[r] - 1, -1) for r in np.argsort(per_rec)[-3:]]
    ids = np.concatenate([ids[:3000], runs[0], ids[3000:], runs[1], runs[2][::2], runs[2]])
    ids = np.concatenate([ids, ids[:700]]).astype(np.int32)            # ... and every early entry again, a tile or more later
    assert len(ids) >= 2 * TILE
    a = int(live[7])
    ids[100:103] = a                                                    # inside one group of 64
    ids[100 + 64 * 5] = a                                               # another wave of the tile
    ids[TILE + 9] = a                                                   # another tile
    b = int(live[11])
    ids[TILE - 1], ids[TILE] = b, b                                     # across the tile boundary
    return ids


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("run_ahead", [0, 1])
def test_by_id_equals_the_oracle(graphs, run_ahead):
    g, o = start(graphs=graphs, run_ahead=run_ahead, oracle=True)
    g.step(3)
    o.step(3)
    ids = mixed_ids(g, o, np.random.default_rng(3))
    r, out = check_by_id(g, o, ids, "by id after 3 steps")
    assert set(np.unique(out)) >= {M.REMOVED, M.NOT_LIVE, M.INVALID} and r["removed"] > 3000
    # a second call finds the claim scratch restored: fresh ids, and all of the first call's again (now not live)
    live = np.nonzero(o.particles["cell"] >= 0)[0]
    ids2 = np.concatenate([live[::3], ids[:2000], live[::3][::-1]]).astype(np.int32)
    r2, _ = check_by_id(g, o, ids2, "second call")
    assert r2["removed"] == len(live[::3])
    g.close()
    o.close()


def test_the_next_steps_match_the_oracle():
    g, o = start(seed=21, oracle=True)
    g.step(2)
    o.step(2)
    rng = np.random.default_rng(21)
    live = np.nonzero(o.particles["cell"] >= 0)[0]
    ids = rng.choice(live, 900).astype(np.int32)            # (with duplicates)
    check_by_id(g, o, ids, "before the steps")
    for k in range(10):
        g.step(1)
        o.step(1)
        assert_same_particles(g.download_particles(), o.particles, "step %d after the remove, vs the oracle" % (k + 1))
    same_as_oracle(g, o, "10 steps after the remove")
    g.close()
    o.close()


def test_crafted_queue_states():
    g, o = start(seed=22, oracle=True)
    g.step(2)
    o.step(2)
    p = o.particles
    qi, q = g.download_queues()
    lo, seg = qi["rloc"].astype(np.int64), qi["seg_size"].astype(np.int64)
    per_rec = np.array([(p["cell"][a:a + s] >= 0).sum() for a, s in zip(lo, seg)])
    ra, rb, rc = (int(r) for r in np.argsort(per_rec)[-3:])
    assert per_rec[[ra, rb, rc]].min() >= 3 and seg[[ra, rb, rc]].min() >= 6 and (seg - per_rec)[rb] >= 2

    def live_of(r, k):
        return (lo[r] + np.nonzero(p["cell"][lo[r]:lo[r] + seg[r]] >= 0)[0][:k]).astype(np.int32)

    def free_of(r, k):
        return (lo[r] + np.nonzero(p["cell"][lo[r]:lo[r] + seg[r]] < 0)[0][:k]).astype(np.int32)
    # a: emptied, as inject or the replay leave a queue they drained
    qi["front"][ra], qi["rear"][ra], qi["count"][ra] = -1, -1, 0
    q[lo[ra]:lo[ra] + seg[ra]] = -1
    # b: two entries, the rear at the segment's last position
    q[lo[rb]:lo[rb] + seg[rb]] = -1
    q[lo[rb] + seg[rb] - 2:lo[rb] + seg[rb]] = free_of(rb, 2)
    qi["front"][rb], qi["rear"][rb], qi["count"][rb] = lo[rb] + seg[rb] - 2, lo[rb] + seg[rb] - 1, 2
    # c: full while some of its slots are live (the cell-overflow rule frees foreign slots into a record)
    q[lo[rc]:lo[rc] + seg[rc]] = np.arange(lo[rc], lo[rc] + seg[rc])
    qi["front"][rc], qi["rear"][rc], qi["count"][rc] = lo[rc], lo[rc] + seg[rc] - 1, seg[rc]
    g.upload_queues(qi, q)
    o.queue_info[:] = qi
    o.queue[:] = q
    same_as_oracle(g, o, "the crafted state")
    ids = np.concatenate([live_of(ra, 3)[::-1], live_of(rb, 3), live_of(rc, 1)])
    full_before = q[lo[rc]:lo[rc] + seg[rc]].copy()
    r, out = check_by_id(g, o, ids, "crafted queue states")
    assert out.tolist() == [0, 0, 0, 0, 0, 0, 4] and r["dropped"] == 1 and r["removed"] == 7
    qi2, q2 = g.download_queues()
    assert tuple(qi2[["front", "rear", "count"]][ra]) == (lo[ra], lo[ra] + 2, 3)
    assert q2[lo[ra]:lo[ra] + 3].tolist() == ids[:3].tolist()
    assert tuple(qi2[["front", "rear", "count"]][rb]) == (lo[rb] + seg[rb] - 2, lo[rb] + 2, 5)
    assert q2[lo[rb]:lo[rb] + 3].tolist() == ids[3:6].tolist()
    assert qi2[rc:rc + 1].tobytes() == qi[rc:rc + 1].tobytes() and np.array_equal(q2[lo[rc]:lo[rc] + seg[rc]], full_before)
    assert g.download_particles()["cell"][ids[6]] == -1
    g.close()
    o.close()


def test_device_count_without_a_sync():
    g, o = start(seed=23, oracle=True)
    g.step(2)
    o.step(2)
    rng = np.random.default_rng(23)
    count = torch.full((1,), 5000, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    live = np.nonzero(o.particles["cell"] >= 0)[0]
    ids = rng.permutation(live)[:5000].astype(np.int32) if len(live) >= 5000 else rng.choice(live, 5000).astype(np.int32)
    with torch.cuda.stream(torch.cuda.ExternalStream(g.stream(), device=DEV)):
        count.fill_(1234)             # written on the context's stream just before the remove: nothing waits for it
        check_by_id(g, o, ids, "device count 1234", count=count, n=1234)
    for c, n in [(0, 0), (-5, 0), (1 << 40, 700)]:
        live = np.nonzero(o.particles["cell"] >= 0)[0]
        ids = rng.choice(live, 700).astype(np.int32)
        count.fill_(c)
        r, _ = check_by_id(g, o, ids, "device count %d" % c, count=count, n=n)
        assert r["done"] == n
    g.step(2)
    o.step(2)
    same_as_oracle(g, o, "2 steps after the device counts")
    g.close()
    o.close()


def upload_a_nan(g, o):
    """x of one live particle is made NaN, in a cell column an upload accepts it in (the index the reference's conversion
    of a NaN lands on, k_unpack_aos)"""
    G = g.sizes.grid_dim
    lost = -(1 << 31)
    while not 0 <= lost < G:
        lost = int(math.fmod(lost + G, G))
    p = g.download_particles()
    cand = np.nonzero((p["cell"] >= 0) & (p["cell"] % G == lost))[0]
    assert len(cand) > 0
    s = int(cand[len(cand) // 2])
    p["x"][s] = np.nan
    g.upload_particles(p)
    o.particles["x"][s] = np.nan
    return s


def inside(pos, lo, hi):
    with np.errstate(invalid="ignore"):
        return ((pos[:, :3] >= np.asarray(lo, np.float32)) & (pos[:, :3] < np.asarray(hi, np.float32))).all(1)


@pytest.mark.parametrize("outside", [False, True])
def test_by_box(outside):
    a, o = start(seed=24, oracle=True)
    b = start(seed=24)
    for s in (a, b, o):
        s.step(3)
    nan_slot = upload_a_nan(a, o)
    b.upload_particles(a.download_particles())
    lo, hi = (-12.5, -40.0, -3.0), (30.0, 9.25, 35.0)          # cuts the cloud
    ex = b.export_live(ps.EXPORT_POS | ps.EXPORT_ID)
    pos, eid = ex["pos4"].cpu().numpy(), ex["id"].cpu().numpy()
    sel = inside(pos, lo, hi) != outside
    assert 100 < sel.sum() < len(sel) - 100 and bool(sel[eid == nan_slot][0]) == outside
    ra = a.remove(box=(lo, hi), outside=outside)
    rb, out = remove_ids(b, eid[sel])
    s_out, s_res = M.serial(o, eid[sel])
    assert (out == 0).all() and (s_out == 0).all()
    want = dict(s_res, done=len(eid))
    assert ra == want and a.remove_result() == ra, (ra, want)
    assert {k: rb[k] for k in ("removed", "dropped")} == {k: ra[k] for k in ("removed", "dropped")}
    same_state(a, b, "by box vs by id of the filtered export")
    same_as_oracle(a, o, "by box vs the oracle")
    # an empty selection changes no byte
    r0 = a.remove(box=((1.0, 1.0, 1.0), (1.0, 1.0, 1.0)))
    assert r0 == dict(done=len(eid) - ra["removed"], removed=0, not_live=0, foreign=0, invalid=0, dropped=0)
    same_as_oracle(a, o, "after an empty selection")
    if outside:          # (the particle without a position is gone: the frames that follow are ordinary ones)
        a.step(2)
        o.step(2)
        same_as_oracle(a, o, "2 steps after the box")
    for s in (a, b, o):
        s.close()


def test_remove_then_inject_into_the_freed_slots():
    g, o = start(seed=25, oracle=True)
    g.step(2)
    o.step(2)
    rng = np.random.default_rng(25)
    live = np.nonzero(o.particles["cell"] >= 0)[0]
    check_by_id(g, o, rng.permutation(live)[:2500].astype(np.int32), "the remove")
    pos4, vel4, fert = batch(g, 3000, 26)
    r = inject(g, pos4, vel4, fert)
    ids = o.fill(pos4[:, :3], age=vel4[:, 3], fert_age=fert, w=pos4[:, 3])
    p = o.particles
    p["vx"][ids], p["vy"][ids], p["vz"][ids] = vel4[:, :3].T
    assert (r["status"], r["done"], r["placed"]) == (OK, 3000, 3000)
    assert np.array_equal(r["ids"], ids), "the ids inject hands out after a remove"
    same_as_oracle(g, o, "remove, then inject")
    g.step(3)
    o.step(3)
    same_as_oracle(g, o, "3 steps after remove + inject")
    g.close()
    o.close()


@pytest.mark.parametrize("world", [2, 3])
def test_slabs(world):
    n = 30000
    xyz = cloud(n, 500 + world)
    rng = np.random.default_rng(world)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    fert = rng.uniform(3.0, 12.0, n).astype(np.float32)
    seed = 50 + world

    def make(**over):
        s = ps.ParticleSystem(ps.default_config(flags=ps.FLAG_EXPLOSIONS, seed=seed, **over))
        s.fill_particles(xyz, age=age, fert_age=fert)
        return s
    ranks = [make(rank=r, world=world) for r in range(world)]
    one = make()
    plans = [s.slab_plan() for s in ranks]

    def same_as_one(what):
        union = merge_owned([s.download_particles() for s in ranks], plans)
        assert_same_particles(union, one.download_particles(), what + ": union vs one context")
        qs = [s.download_queues() for s in ranks]
        qi1, q1 = one.download_queues()
        assert merge_owned([x[0] for x in qs], plans, "records").tobytes() == qi1.tobytes(), what + ": QUEUE_INFO records"
        assert np.array_equal(merge_owned([x[1] for x in qs], plans), q1), what + ": queues"
    for _ in range(2):
        step_local(ranks)
    one.step(2)
    cont = one.sizes.container_size
    cell = one.download_particles()["cell"]
    live, free = np.nonzero(cell >= 0)[0], np.nonzero(cell < 0)[0]
    ids = np.concatenate([rng.choice(live, 9000), rng.choice(free, 500), [-3, cont, cont + 7]]).astype(np.int32)
    rng.shuffle(ids)
    r1, out1 = remove_ids(one, ids)
    total = dict.fromkeys(M.RESULT_KEYS, 0)
    valid = (ids >= 0) & (ids < cont)
    for rank, (s, pl) in enumerate(zip(ranks, plans)):          # every rank is given the whole list and removes its own
        owned = np.zeros(cont, bool)
        for t in range(4):
            owned[pl.slot_lo[t]:pl.slot_hi[t]] = True
        mine = valid & owned[np.where(valid, ids, 0)]
        r, out = remove_ids(s, ids)
        assert r["foreign"] == int((valid & ~mine).sum()) and r["invalid"] == 3 and r["done"] == len(ids), (rank, r)
        assert np.array_equal(out[mine], out1[mine]) and (out[valid & ~mine] == M.FOREIGN).all(), rank
        for k in total:
            total[k] += r[k]
    assert total == ps.merge_remove([dict(r1, done=world * len(ids), invalid=3 * world,
                                          foreign=(world - 1) * int(valid.sum()))])
    same_as_one("world %d by id" % world)
    box = ((-40.0, -15.0, -40.0), (40.0, 40.0, 11.0))
    rb1 = one.remove(box=box, outside=True)
    rbs = ps.merge_remove(s.remove(box=box, outside=True) for s in ranks)
    assert rbs == rb1 and 1000 < rb1["removed"] < rb1["done"], (rbs, rb1)
    same_as_one("world %d by box" % world)
    for k in range(3):
        step_local(ranks)
        one.step(1)
        same_as_one("world %d step %d" % (world, k + 1))
    for s in ranks + [one]:
        s.close()


def test_arguments_capture_and_the_frame():
    a, b = start(seed=28), start(seed=28)
    a.step(1)
    b.step(1)
    ids = torch.arange(0, 1001, dtype=torch.int32, device=DEV)
    out = torch.zeros(1001, dtype=torch.int32, device=DEV)
    res = torch.zeros(8, dtype=torch.int64, device=DEV)
    cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()

    def spec(**over):
        s = ps.Remove(max_count=1000, ids=ids.data_ptr(), outcome_dev=out.data_ptr())
        for k, v in over.items():
            setattr(s, k, v)
        return s

    def box(**over):
        s = ps.Remove(flags=ps.REMOVE_BOX)
        for k, v in over.items():
            setattr(s, k, v)
        return s
    lib = b.lib
    assert lib.psamd_remove(None, C.byref(spec())) == ERR_INVALID_ARG
    assert lib.psamd_remove(b.h, None) == ERR_INVALID_ARG
    assert lib.psamd_remove_result_get(b.h, None) == ERR_INVALID_ARG
    for bad in (spec(flags=4), spec(flags=ps.REMOVE_OUTSIDE), spec(reserved=1), spec(max_count=-1), spec(max_count=1 << 31),
                spec(ids=None), spec(ids=ids.data_ptr() + 2), spec(outcome_dev=out.data_ptr() + 2),
                spec(count_dev=cnt.data_ptr() + 4), spec(result_dev=res.data_ptr() + 4),
                box(flags=ps.REMOVE_BOX | 8), box(reserved=1), box(ids=ids.data_ptr()), box(count_dev=cnt.data_ptr()),
                box(outcome_dev=out.data_ptr()), box(max_count=1), box(result_dev=res.data_ptr() + 4)):
        assert lib.psamd_remove(b.h, C.byref(bad)) == ERR_INVALID_ARG, [(n, getattr(bad, n)) for n, _ in bad._fields_[:6]]
    same_state(a, b, "after the refused calls")
    # max_count == 0: a zero result, nothing else
    assert b.remove(ids=ids[:1000].contiguous())["done"] == 1000
    a.remove(ids=ids[:1000].contiguous())
    res.fill_(-1)
    torch.cuda.synchronize()
    assert lib.psamd_remove(b.h, C.byref(spec(max_count=0, ids=None, outcome_dev=None, result_dev=res.data_ptr()))) == OK
    assert b.remove_result() == dict.fromkeys(M.RESULT_KEYS, 0)
    assert res[:6].cpu().tolist() == [0] * 6
    same_state(a, b, "max_count 0")
    # capture: refused, the graph stays empty, the state untouched
    with captured(b) as cap:
        rc = lib.psamd_remove(b.h, C.byref(spec(ids=ids.data_ptr() + 4)))
        rc2 = lib.psamd_remove(b.h, C.byref(box()))
    assert rc == ERR_STATE and rc2 == ERR_STATE, (rc, rc2)
    assert b"captured" in lib.psamd_last_error(b.h)
    assert cap.nodes() == 0
    cap.close()
    same_state(a, b, "after the refused capture")
    # a remove between build_grid and calc_forces ends the frame
    for g in (a, b):
        g.init_iframe()
        g.build_grid()
    assert b.remove(ids=ids[1:1001].contiguous())["done"] == 1000
    a.remove(ids=ids[1:1001].contiguous())
    assert lib.psamd_calc_forces(b.h) == ERR_STATE and lib.psamd_calc_forces_pairs(b.h) == ERR_STATE
    for g in (a, b):
        g.init_iframe()
        g.build_grid()
        g.calc_forces()
    same_state(a, b, "a frame after the refused calc_forces")
    for g in (a, b):
        g.close()


def test_snapshot_after_a_remove():
    g, o = start(seed=29, oracle=True)
    g.step(2)
    o.step(2)
    live = np.nonzero(o.particles["cell"] >= 0)[0]
    check_by_id(g, o, live[::2].astype(np.int32), "the remove")
    g.snapshot_save()
    saved = state(g)
    g.step(1)
    o.step(1)
    same_as_oracle(g, o, "the step after the save")
    g.snapshot_restore()
    p, qi, q = state(g)
    assert_same_particles(p, saved[0], "restored particles")
    assert qi.tobytes() == saved[1].tobytes() and np.array_equal(q, saved[2])
    g.close()
    o.close()


def same_as_model(g, want, what):
    for got, w, name in zip(state(g), want, ("particles", "QUEUE_INFO records", "queues")):
        assert got.tobytes() == w.tobytes(), "%s: %s differ" % (what, name)


@pytest.mark.parametrize("outside", [False, True])
def test_by_box_ragged_last_tile(outside):
    """18 000 owned slots: four slot tiles and one of 1616, the selection in all five"""
    g, rec = ragged(seed=35)
    lo, hi = (-12.5, -20.0, -3.0), (15.0, 9.25, 20.0)
    sel = inside(np.stack([rec["x"], rec["y"], rec["z"]], 1), lo, hi) != outside
    ids = rec["id"][sel].astype(np.int32)
    assert set(ids // SLOT_TILE) == set(range((g.owned_slots() + SLOT_TILE - 1) // SLOT_TILE)) and 0 < len(ids) < len(rec)
    p2, qi2, q2, out, want = M.closed_form(g.sizes, g.sizes.num_cells, *state(g), ids)
    assert (out == M.REMOVED).all()
    r = g.remove(box=(lo, hi), outside=outside)
    assert r == dict(want, done=len(rec)) and g.remove_result() == r, (r, want)
    same_as_model(g, (p2, qi2, q2), "by box, ragged last tile")
    g.close()


def test_by_id_with_more_than_8192_queue_records():
    """9261 records: the tile counts in global memory; three tiles of entries, the last one ragged"""
    g = many_records()
    pos4, vel4, fert = batch(g, 8192 + 100, 42)
    assert inject(g, pos4, vel4, fert)["placed"] == len(pos4)
    p, qi, q = state(g)
    live = np.nonzero(p["cell"] >= 0)[0]
    free = np.nonzero(p["cell"] < 0)[0]
    rng = np.random.default_rng(42)
    ids = np.concatenate([live, rng.choice(live, 60), [g.sizes.container_size, int(free[len(free) // 2])]]).astype(np.int32)
    rng.shuffle(ids)
    assert len(ids) >= 8193 and len(ids) % TILE != 0
    p2, qi2, q2, s_out, want = M.closed_form(g.sizes, g.sizes.num_cells, p, qi, q, ids)
    r, out = remove_ids(g, ids)
    assert np.array_equal(out, s_out), np.nonzero(out != s_out)[0][:10]
    assert r == want and want["removed"] == len(live) and want["invalid"] == 1 and want["not_live"] == 61, (r, want)
    same_as_model(g, (p2, qi2, q2), "by id, 9261 records")
    g.close()
