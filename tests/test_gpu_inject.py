"""Putting particles in (psamd_inject / psamd_inject_result_get, inject.hip): the device-side, stream-ordered
psamd_fill_particles.  What must hold: after an inject, the particle arrays, the queues and their records, the ids,
done, placed and the status are byte-equal to what fill_particles leaves with the same batch at the same point of the
stream -- with graphs on and off, run-ahead 0 and 1, on slabs, with a device-written count, at every stop (outside the
box, a queue that runs empty) -- and the steps that follow stay equal, also in all-pairs mode with run-ahead 1 (the
host's live bound)."""
import ctypes as C

import numpy as np
import pytest
import torch

import particlesystem_amd as ps
from particlesystem_amd.slab import merge_owned, step_local
from service_harness import (DEV, ERR_INVALID_ARG, ERR_OUTSIDE_BOX, ERR_QUEUE_EMPTY, ERR_STATE, OK, batch, captured, dev, fill, inject,
                             many_records, same_as_fill, same_state, start)
from util import assert_same_particles, cloud

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("run_ahead", [0, 1])
def test_inject_equals_fill(graphs, run_ahead):
    a, b = start(graphs=graphs, run_ahead=run_ahead), start(graphs=graphs, run_ahead=run_ahead)
    a.step(3)
    b.step(3)
    pos4, vel4, fert = batch(a, 20000, 5)
    f = fill(a, pos4, vel4, fert)
    r = inject(b, pos4, vel4, fert)
    assert f[0] == OK and f[1] == len(pos4)
    same_as_fill(f, r, "inject after 3 steps")
    assert b.inject_result() == {k: r[k] for k in ("done", "placed", "status")}
    same_state(a, b, "inject after 3 steps")
    # the optional inputs left out: velocity and age 0, fertility age 0
    pos4, _, _ = batch(a, 3000, 6)
    same_as_fill(fill(a, pos4), inject(b, pos4), "positions only")
    same_state(a, b, "positions only")
    a.close()
    b.close()


@pytest.mark.parametrize("run_ahead", [0, 1])
def test_the_next_steps_match(run_ahead):
    a, b = start(seed=12, run_ahead=run_ahead), start(seed=12, run_ahead=run_ahead)
    a.step(2)
    b.step(2)
    pos4, vel4, fert = batch(a, 40000, 7)
    fill(a, pos4, vel4, fert)
    inject(b, pos4, vel4, fert)
    for k in range(10):
        a.step(1)
        b.step(1)
        same_state(a, b, "step %d after the inject" % (k + 1))
    a.close()
    b.close()


def test_the_next_steps_match_the_oracle():
    g, o = start(seed=13, oracle=True)
    g.step(2)
    o.step(2)
    pos4, vel4, fert = batch(g, 600, 8)
    r = inject(g, pos4, vel4, fert)
    ids = o.fill(pos4[:, :3], age=vel4[:, 3], fert_age=fert, w=pos4[:, 3])
    p = o.particles
    p["vx"][ids], p["vy"][ids], p["vz"][ids] = vel4[:, :3].T
    assert (r["status"], r["done"], r["placed"]) == (OK, 600, 600) and np.array_equal(r["ids"], ids)
    assert_same_particles(g.download_particles(), o.particles, "inject vs oracle fill")
    for k in range(10):
        g.step(1)
        o.step(1)
        assert_same_particles(g.download_particles(), o.particles, "step %d after the inject, vs the oracle" % (k + 1))
    qi, q = g.download_queues()
    assert qi.tobytes() == o.queue_info.tobytes() and np.array_equal(q, o.queue)
    g.close()
    o.close()


def test_stops_where_fill_stops():
    a, b = start(seed=14), start(seed=14)
    a.step(2)
    b.step(2)
    base, vel4, fert = batch(a, 9000, 9)
    for k, (i, bad) in enumerate([(4000, (1e5, 0.0, 0.0)), (700, (np.nan, 1.0, 1.0)), (5000, (0.0, np.inf, 0.0)),
                                  (1, (0.0, 0.0, -np.inf)), (8999, (1e30, 0.0, 0.0)), (3333, (0.0, 0.0, -1e30)),
                                  (0, (0.0, -1e30, 0.0))]):
        pos4 = base.copy()
        pos4[i, :3] = bad
        f = fill(a, pos4, vel4, fert)
        r = inject(b, pos4, vel4, fert)
        assert f[0] == ERR_OUTSIDE_BOX and f[1] == i, (k, f[:2])
        same_as_fill(f, r, "outside entry %r at %d" % (bad, i))
        same_state(a, b, "outside entry %r at %d" % (bad, i))
        base, vel4, fert = batch(a, 9000, 20 + k)
    # a batch aimed into one segment beyond its free count, between ordinary entries
    qi, _ = a.download_queues()
    m = int(qi["seg_size"].max()) + 10
    head, _, _ = batch(a, 500, 30)
    tail, _, _ = batch(a, 100, 31)
    spot = np.repeat(head[:1], m, 0)
    pos4 = np.ascontiguousarray(np.concatenate([head, spot, tail]))
    rng = np.random.default_rng(32)
    vel4 = rng.uniform(-5, 5, (len(pos4), 4)).astype(np.float32)
    fert = rng.uniform(3.0, 12.0, len(pos4)).astype(np.float32)
    f = fill(a, pos4, vel4, fert)
    r = inject(b, pos4, vel4, fert)
    assert f[0] == ERR_QUEUE_EMPTY and 500 <= f[1] < 500 + m, f[:2]
    same_as_fill(f, r, "queue runs empty")
    same_state(a, b, "queue runs empty")
    a.step(3)
    b.step(3)
    same_state(a, b, "3 steps after the stops")
    a.close()
    b.close()


def test_device_count_without_a_sync():
    a, b = start(seed=15), start(seed=15)
    a.step(2)
    b.step(2)
    pos4, vel4, fert = batch(a, 12000, 10)
    count = torch.full((1,), 12000, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.ExternalStream(b.stream(), device=DEV)):
        count.fill_(7777)             # written on the context's stream just before the inject: nothing waits for it
        r = inject(b, pos4, vel4, fert, count=count)
    f = fill(a, pos4[:7777], vel4[:7777], fert[:7777])
    same_as_fill(f, r, "device count 7777")
    assert (r["ids"][7777:] == -1).all()
    same_state(a, b, "device count 7777")
    # clamped: 0, negative, above max_count
    for k, (c, n) in enumerate([(0, 0), (-5, 0), (1 << 40, 3000)]):
        pos4, vel4, fert = batch(a, 3000, 40 + k)
        count.fill_(c)
        r = inject(b, pos4, vel4, fert, count=count)
        f = fill(a, pos4[:n], vel4[:n], fert[:n])
        same_as_fill(f, r, "device count %d" % c)
        same_state(a, b, "device count %d" % c)
    a.step(2)
    b.step(2)
    same_state(a, b, "2 steps after the device counts")
    a.close()
    b.close()


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
    filled = [make(rank=r, world=world) for r in range(world)]
    injected = [make(rank=r, world=world) for r in range(world)]
    one = make()
    for _ in range(3):
        step_local(filled)
        step_local(injected)
    one.step(3)
    pos4, vel4, bfert = batch(one, 20000, 60 + world)
    placed = 0
    for rank, (a, b) in enumerate(zip(filled, injected)):      # every rank is given the whole batch and keeps its own entries
        f = fill(a, pos4, vel4, bfert)
        r = inject(b, pos4, vel4, bfert)
        same_as_fill(f, r, "rank %d of %d" % (rank, world))
        assert r["done"] == len(pos4)
        placed += r["placed"]
        same_state(a, b, "world %d rank %d" % (world, rank))
    r1 = inject(one, pos4, vel4, bfert)
    assert r1["placed"] == placed == len(pos4) and r1["status"] == OK
    for k in range(6):
        step_local(filled)
        step_local(injected)
        one.step(1)
        for a, b in zip(filled, injected):
            same_state(a, b, "world %d step %d" % (world, k + 1))
        union = merge_owned([s.download_particles() for s in injected], [s.slab_plan() for s in injected])
        assert_same_particles(union, one.download_particles(), "world %d step %d: union vs one context" % (world, k + 1))
    for s in filled + injected + [one]:
        s.close()


def test_all_pairs_live_bound_with_run_ahead():
    """a step enqueued, then a large inject, then steps, with no sync: the far pass must cover the injected particles
    although the host reads the record of a step enqueued before the inject afterwards"""
    def make():
        g = ps.ParticleSystem(ps.default_config(flags=ps.FLAG_ALL_PAIRS, seed=3))
        g.set_run_ahead(1)
        g.fill_particles(cloud(40, 77), age=np.float32(1.0), fert_age=np.float32(1e6))
        return g
    a, b = make(), make()
    pos4, vel4, fert = batch(a, 20000, 70)
    vel4[:, 3] = 1.0
    fert[:] = 1e6
    for g in (a, b):
        assert g.lib.psamd_step(g.h, 1) == 0
        spec = ps.Inject(max_count=len(pos4))
        tp, tv, tf = dev(pos4), dev(vel4), dev(fert)
        spec.pos4, spec.vel4, spec.fert_age = tp.data_ptr(), tv.data_ptr(), tf.data_ptr()
        torch.cuda.synchronize()
        assert g.lib.psamd_inject(g.h, C.byref(spec)) == 0
        if g is a:
            assert g.lib.psamd_step(g.h, 4) == 0      # enqueued behind the inject, no sync in between
        g.synchronize()
        g._keep = (tp, tv, tf)
    assert a.inject_result() == {"done": 20000, "placed": 20000, "status": OK}
    # b: the state right after the inject, uploaded into a fresh context (upload: every owned slot is covered)
    p, (qi, q) = b.download_particles(), b.download_queues()
    c = ps.ParticleSystem(ps.default_config(flags=ps.FLAG_ALL_PAIRS, seed=3))
    c.upload_particles(p)
    c.upload_queues(qi, q)
    c.step(4)
    same_state(a, c, "all-pairs, 4 steps after the inject")
    for g in (a, b, c):
        g.close()


def test_export_round_trip():
    a = start(seed=17)
    a.step(4)
    ex = a.export_live(ps.EXPORT_POS | ps.EXPORT_VEL | ps.EXPORT_ACC)
    fert = ex["acc4"][:, 3].contiguous()
    b = ps.ParticleSystem(ps.default_config(flags=ps.FLAG_EXPLOSIONS, seed=17))
    c = ps.ParticleSystem(ps.default_config(flags=ps.FLAG_EXPLOSIONS, seed=17))
    r = b.inject(ex["pos4"].contiguous(), ex["vel4"].contiguous(), fert, ids=True)
    f = fill(c, ex["pos4"].cpu().numpy(), ex["vel4"].cpu().numpy(), fert.cpu().numpy())
    r["ids"] = r["ids"].cpu().numpy()
    same_as_fill(f, r, "export round trip")
    assert r["done"] == ex["count"]
    same_state(b, c, "export round trip")
    for g in (a, b, c):
        g.close()


def test_arguments_and_capture():
    a, b = start(seed=18), start(seed=18)
    a.step(1)
    b.step(1)
    pos4, vel4, fert = batch(a, 1000, 80)
    tp, tv, tf = dev(pos4), dev(vel4), dev(fert)
    ids = torch.zeros(1001, dtype=torch.int32, device=DEV)
    res = torch.zeros(8, dtype=torch.int64, device=DEV)
    cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
    raw = torch.zeros(1000 * 4 + 4, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()

    def spec(**over):
        s = ps.Inject(max_count=1000, pos4=tp.data_ptr(), vel4=tv.data_ptr(), fert_age=tf.data_ptr(), ids_dev=ids.data_ptr())
        for k, v in over.items():
            setattr(s, k, v)
        return s
    lib = b.lib
    assert lib.psamd_inject(None, C.byref(spec())) == ERR_INVALID_ARG
    assert lib.psamd_inject(b.h, None) == ERR_INVALID_ARG
    for bad in (dict(flags=1), dict(reserved=1), dict(max_count=-1), dict(max_count=1 << 31), dict(pos4=None),
                dict(pos4=raw.data_ptr() + 4), dict(vel4=raw.data_ptr() + 8), dict(fert_age=tf.data_ptr() + 2),
                dict(ids_dev=ids.data_ptr() + 2), dict(result_dev=res.data_ptr() + 4), dict(count_dev=cnt.data_ptr() + 4)):
        assert lib.psamd_inject(b.h, C.byref(spec(**bad))) == ERR_INVALID_ARG, bad
    assert lib.psamd_inject_result_get(b.h, None) == ERR_INVALID_ARG
    # max_count == 0: a zero result, nothing else
    r0 = inject(b, pos4, vel4, fert)
    assert r0["done"] == 1000
    fill(a, pos4, vel4, fert)
    res.fill_(-1)
    torch.cuda.synchronize()
    assert lib.psamd_inject(b.h, C.byref(spec(max_count=0, result_dev=res.data_ptr()))) == OK
    assert b.inject_result() == {"done": 0, "placed": 0, "status": OK}
    assert res[:3].cpu().tolist() == [0, 0, 0]
    same_state(a, b, "max_count 0")
    # capture: refused, the graph stays empty, the state untouched
    with captured(b) as cap:
        rc = lib.psamd_inject(b.h, C.byref(spec()))
    assert rc == ERR_STATE, rc
    assert b"captured" in lib.psamd_last_error(b.h)
    assert cap.nodes() == 0
    cap.close()
    same_state(a, b, "after the refused capture")
    a.step(2)
    b.step(2)
    same_state(a, b, "2 steps after the refused capture")
    for g in (a, b):
        g.close()


# ---- more queue records than the tile's counts have room for in LDS (service_harness.many_records) -------------------------------

def test_more_than_8192_queue_records():
    a, b = many_records(), many_records()
    pos4, vel4, fert = batch(a, 8192 + 100, 41)          # three tiles of entries, the last one ragged
    f = fill(a, pos4, vel4, fert)
    r = inject(b, pos4, vel4, fert)
    assert f[0] == OK and f[1] == len(pos4)
    same_as_fill(f, r, "9261 records")
    same_state(a, b, "9261 records")
    a.close()
    b.close()
