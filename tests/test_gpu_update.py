"""Changing particles in place (psamd_update / psamd_update_result_get, update.hip).  What must hold: after an update the
particle arrays are byte-equal to the serial definition (tests/update_model.py) applied to the download made before the
call -- by id and by export order, for every field set, with graphs on and off, run-ahead 0 and 1, with a device-written
count, on a container whose last slot tile is ragged, on slabs; the queues and their records are untouched; the claim words
are left as they were found; the steps that follow a kick equal those of a context that got the same edit through
download_particles / upload_particles, wherever in the frame the kick is placed; and the frame rules of the header."""
import ctypes as C

import numpy as np
import pytest
import torch

import particlesystem_amd as ps
import remove_model as R
import update_model as U
from particlesystem_amd.slab import merge_owned, step_local
from service_harness import DEV, ERR_INVALID_ARG, ERR_STATE, OK, captured, dev, start, state
from util import SLOT_TILE, assert_same_particles, cloud, ragged

pytestmark = pytest.mark.gpu

TILE = 4096          # the tile of entries (ENTRY_TILE)
VEL, AGE, MASS, FERT, ADD, ORDER = U.VEL, U.AGE, U.MASS, U.FERT, U.ADD, U.EXPORT_ORDER
FIELD_SETS = (VEL, VEL | ADD, MASS | AGE | FERT, VEL | AGE | MASS | FERT)


def entries(m, seed):
    """vel4 (vx, vy, vz, age), w, fert_age for m entries: finite, every entry different"""
    rng = np.random.default_rng(seed)
    vel4 = np.concatenate([rng.uniform(-30, 30, (m, 3)), rng.uniform(0.0, 9.0, (m, 1))], 1).astype(np.float32)
    return np.ascontiguousarray(vel4), rng.uniform(0.5, 90.0, m).astype(np.float32), rng.uniform(3.0, 12.0, m).astype(np.float32)


def update(g, fields, ids=None, vel4=None, w=None, fert=None, count=None):
    """g.update with exactly the arrays the fields name: (result, outcomes)"""
    r = g.update(ids=dev(ids), vel4=dev(vel4) if fields & (VEL | AGE) else None, w=dev(w) if fields & MASS else None,
                 fert_age=dev(fert) if fields & FERT else None, count=count, outcome=True, fields=fields)
    out = r.pop("outcome").cpu().numpy()
    return r, out


def check(g, fields, what, ids=None, vel4=None, w=None, fert=None, count=None, n=None, owned=None, before=None):
    """the update on the GPU, the model on the download made before it (before: that download, where the caller has made
    it): everything equal, the queues untouched"""
    m = len(next(a for a in (ids, vel4, w, fert) if a is not None))
    n = m if n is None else n
    p0, qi0, q0 = state(g) if before is None else before
    want, s_out, s_res = U.apply(p0, g.sizes.num_cells, fields, ids, vel4, w, fert, n=n, owned=owned)
    r, out = update(g, fields, ids, vel4, w, fert, count)
    p1, qi1, q1 = state(g)
    assert np.array_equal(out[:n], s_out), (what, np.nonzero(out[:n] != s_out)[0][:10])
    assert (out[n:] == -1).all(), what + ": outcomes past n"
    assert r == s_res, (what, r, s_res)
    assert g.update_result() == r
    assert_same_particles(p1, want, what + ": particles against the model")
    assert qi1.tobytes() == qi0.tobytes() and q1.tobytes() == q0.tobytes(), what + ": the queues changed"
    return r, out


def mixed_ids(g, rng):
    """at least two tiles: live ids, free slots, invalid ids, duplicates inside a 64-entry group, across the waves of a
    tile and across the tile boundary"""
    cont = g.sizes.container_size
    cell = g.download_particles()["cell"]
    live, free = np.nonzero(cell >= 0)[0], np.nonzero(cell < 0)[0]
    ids = np.concatenate([rng.permutation(live)[:3000], rng.choice(live, 3500), rng.choice(free, 1500), rng.integers(-1000, 0, 60),
                          rng.integers(cont, cont + 1000, 60), [np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1, cont, 0, cont - 1]])
    rng.shuffle(ids)
    ids = np.concatenate([ids, ids[:700]]).astype(np.int32)            # ... and every early entry again, two tiles later
    assert len(ids) >= 2 * TILE and len(ids) % TILE != 0
    a = int(live[7])
    ids[100:103] = a                                                    # inside one group of 64
    ids[100 + 64 * 5] = a                                               # another wave of the tile
    ids[TILE + 9] = a                                                   # another tile
    b = int(live[11])
    ids[TILE - 1], ids[TILE] = b, b                                     # across the tile boundary
    return ids


# ---- 1: by id equals the model ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("run_ahead", [0, 1])
def test_by_id_equals_the_model(graphs, run_ahead):
    g = start(graphs=graphs, run_ahead=run_ahead)
    g.step(3)
    rng = np.random.default_rng(3)
    ids = mixed_ids(g, rng)
    for k, fields in enumerate(FIELD_SETS):                             # (every call after the first finds the claims restored)
        vel4, w, fert = entries(len(ids), 10 + k)
        r, out = check(g, fields, "by id, fields %#x" % fields, ids, vel4, w, fert)
        assert set(np.unique(out)) == {U.UPDATED, U.NOT_LIVE, U.INVALID, U.DUPLICATE} and r["updated"] > 3000 and r["duplicate"] > 700
    # a device count: the entries past it keep what they had
    count = torch.full((1,), len(ids) - 900, dtype=torch.int64, device=DEV)
    vel4, w, fert = entries(len(ids), 20)
    check(g, VEL | ADD | FERT, "by id with a count", ids, vel4, w, fert, count=count, n=len(ids) - 900)
    # a remove behind the updates finds the claim words as it left them, and an update behind the remove too
    p2, qi2, q2, s_out, want = R.closed_form(g.sizes, g.sizes.num_cells, *state(g), ids)
    rr = g.remove(ids=dev(ids), outcome=True)
    assert np.array_equal(rr.pop("outcome").cpu().numpy(), s_out) and rr == want and want["removed"] > 3000
    for got, wnt, name in zip(state(g), (p2, qi2, q2), ("particles", "QUEUE_INFO records", "queues")):
        assert got.tobytes() == wnt.tobytes(), "the remove behind the updates: %s differ" % name
    r, out = check(g, VEL | AGE, "an update behind the remove", ids, *entries(len(ids), 21))
    assert r["updated"] == 0 and set(np.unique(out)) == {U.NOT_LIVE, U.INVALID}
    g.step(2)
    g.synchronize()
    g.close()


# ---- 2: by export order -------------------------------------------------------------------------------------------------------------

def test_by_export_order():
    """18 000 owned slots: four slot tiles and one of 1616; holes in every tile"""
    g, rec = ragged(seed=36)
    g.remove(ids=dev(rec["id"][::3].astype(np.int32)))
    ex = g.export_live(ps.EXPORT_ID)
    eid = ex["id"].cpu().numpy()
    live = ex["count"]
    assert live == len(rec) - len(rec[::3]) and set(eid // SLOT_TILE) == set(range((g.owned_slots() + SLOT_TILE - 1) // SLOT_TILE))
    assert g.owned_slots() % SLOT_TILE != 0
    m = live + 300
    for k, (n, fields) in enumerate([(live - 77, VEL), (live, VEL | ADD), (m, VEL | AGE | MASS | FERT), (1, MASS | AGE | FERT), (0, FERT)]):
        vel4, w, fert = entries(m, 30 + k)
        count = torch.full((1,), n, dtype=torch.int64, device=DEV)
        r, out = check(g, fields, "export order, n = %d" % n, None, vel4, w, fert, count=count, n=n)
        assert r["updated"] == min(n, live) and r["not_live"] == max(0, n - live)
    # no count: all m entries, the last 300 find no particle
    vel4, w, fert = entries(m, 40)
    r, out = check(g, VEL | AGE, "export order, no count", None, vel4, w, fert)
    assert (r["done"], r["updated"], r["not_live"]) == (m, live, 300) and (out[live:] == U.NOT_LIVE).all()
    # particle k of an export made just before is the one that got entry k
    ex = g.export_live(ps.EXPORT_ID | ps.EXPORT_VEL)
    assert np.array_equal(ex["id"].cpu().numpy(), eid) and np.array_equal(ex["vel4"].cpu().numpy(), vel4[:live])
    # a count written on the stream just before the call: nothing waits for it
    count = torch.full((1,), m, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    vel4, w, fert = entries(m, 41)
    before = state(g)
    with torch.cuda.stream(torch.cuda.ExternalStream(g.stream(), device=DEV)):
        count.fill_(1234)
        check(g, VEL | ADD, "export order, a device count of 1234", None, vel4, w, fert, count=count, n=1234, before=before)
    g.close()


# ---- 3: SET writes bits ----------------------------------------------------------------------------------------------------------------

def test_set_writes_the_bits_it_is_given():
    g = start(seed=14)
    g.step(2)
    words = np.array([0x7fc00001, 0xffc12345, 0x7fa00000, 0xff800001, 0x80000000, 0x00000000, 0x7f800000, 0xff800000,
                      0x00000001, 0x807fffff, 0x00800000, 0x7f7fffff], np.uint32)
    cell = g.download_particles()["cell"]
    live = np.nonzero(cell >= 0)[0]
    rng = np.random.default_rng(14)
    ids = rng.permutation(live)[:len(words) * 20].astype(np.int32)
    m = len(ids)
    vel4 = np.zeros((m, 4), np.float32)
    for c in range(4):
        vel4.view(np.uint32)[:, c] = np.roll(np.tile(words, 20), c)
    w = np.roll(np.tile(words, 20), 5).view(np.float32)
    fert = np.roll(np.tile(words, 20), 7).view(np.float32)
    check(g, VEL | AGE | MASS | FERT, "special words by id", ids, vel4, w, fert)
    p = g.download_particles()
    for c, f in enumerate(("vx", "vy", "vz", "age")):
        assert np.array_equal(p[f].view(np.uint32)[ids], vel4.view(np.uint32)[:, c]), f
    assert np.array_equal(p["w"].view(np.uint32)[ids], w.view(np.uint32)) and np.array_equal(p["fertility_age"].view(np.uint32)[ids], fert.view(np.uint32))
    check(g, VEL, "special words by export order, velocity alone", None, vel4[::-1].copy())
    check(g, AGE, "special words, age alone", ids, vel4)
    check(g, MASS, "special words by export order, mass alone", None, None, w, fert)
    g.close()


# ---- 4: the steps that follow ----------------------------------------------------------------------------------------------------------

def test_the_steps_after_a_kick_wherever_it_is_placed():
    a, b, c, d = (start(seed=15) for _ in range(4))
    for s in (a, b, c, d):
        s.step(2)
    p = b.download_particles()
    live = np.nonzero(p["cell"] >= 0)[0]
    rng = np.random.default_rng(15)
    ids = rng.permutation(live)[:3000].astype(np.int32)
    kick = np.ascontiguousarray(np.concatenate([rng.uniform(-5, 5, (3000, 3)), np.zeros((3000, 1))], 1).astype(np.float32))
    # b: the host route at the same point
    for k, f in enumerate(("vx", "vy", "vz")):
        p[f][ids] = p[f][ids] + kick[:, k]
    b.upload_particles(p)
    # a: between frames; c: behind build_grid; d: behind the pair stage (which reads no velocity)
    assert update(a, VEL | ADD, ids, kick)[0]["updated"] == 3000
    assert_same_particles(a.download_particles(), b.download_particles(), "the kick against the host route")
    a.step(1)
    b.step(1)
    c.init_iframe(); c.build_grid()
    assert update(c, VEL | ADD, ids, kick)[0]["updated"] == 3000
    c.calc_forces()
    d.init_iframe(); d.build_grid(); d.calc_forces_pairs()
    assert update(d, VEL | ADD, ids, kick)[0]["updated"] == 3000
    d.calc_forces_apply()
    for k in range(5):
        if k:
            for s in (a, b, c, d):
                s.step(1)
        want = b.download_particles()
        for s, name in ((a, "at ST_IDLE"), (c, "behind build_grid"), (d, "behind calc_forces_pairs")):
            assert_same_particles(s.download_particles(), want, "step %d after a kick %s, against the host route" % (k + 1, name))
    for s in (a, b, c, d):
        s.close()


# ---- 5: the frame rules ----------------------------------------------------------------------------------------------------------------

def raw(g, fields, m, ids=None, vel4=None, w=None, fert=None, **over):
    spec = ps.Update(fields=fields, max_count=m)
    for name, t in (("ids", ids), ("vel4", vel4), ("w", w), ("fert_age", fert)):
        setattr(spec, name, None if t is None else t.data_ptr())
    for k, v in over.items():
        setattr(spec, k, v)
    return g.lib.psamd_update(g.h, C.byref(spec))


def test_the_frame_rules_and_capture():
    g = start(seed=16)
    g.step(1)
    live = np.nonzero(g.download_particles()["cell"] >= 0)[0]
    ids_np = live[:2000].astype(np.int32)
    vel_np, w_np, fert_np = entries(2000, 16)
    vel_np[:, :3] *= 0.1
    ids, vel4, w, fert = dev(ids_np), dev(vel_np), dev(w_np), dev(fert_np)
    lib = g.lib
    # velocity and fertility age are not in the snapshot: the frame goes on
    for fields in (VEL, VEL | ADD, FERT, VEL | ADD | FERT | ORDER):
        g.init_iframe(); g.build_grid()
        r = g.update(ids=None if fields & ORDER else ids, vel4=vel4, fert_age=fert, fields=fields)
        assert r["done"] == 2000 and r["updated"] > 1000, r        # (the steps in between let some of the 2000 die)
        assert lib.psamd_calc_forces(g.h) == OK, hex(fields)
    # mass and age are: the frame is over
    for fields in (MASS, AGE, VEL | MASS, AGE | ORDER):
        g.init_iframe(); g.build_grid()
        r = g.update(ids=None if fields & ORDER else ids, vel4=vel4, w=w, fields=fields)
        assert r["done"] == 2000 and r["updated"] > 1000, r
        assert lib.psamd_calc_forces(g.h) == ERR_STATE and lib.psamd_calc_forces_pairs(g.h) == ERR_STATE, hex(fields)
        g.init_iframe(); g.build_grid(); g.calc_forces()
    # a kick captured into a graph, by id and by export order (no scratch grows: 2000 entries were served above); every replay kicks once
    p0 = g.download_particles()
    with captured(g) as cap:
        rc = raw(g, VEL | ADD, 2000, ids, vel4)
        rc2 = raw(g, VEL | ADD | ORDER, 1500, None, vel4)
    assert (rc, rc2) == (OK, OK), (rc, rc2)
    assert g.download_particles().tobytes() == p0.tobytes(), "a capture runs nothing"
    want = p0
    for k in range(3):
        cap.launch()
        want = U.apply(want, g.sizes.num_cells, VEL | ADD, ids_np, vel_np)[0]
        want = U.apply(want, g.sizes.num_cells, VEL | ADD, None, vel_np[:1500])[0]
        assert_same_particles(g.download_particles(), want, "replay %d of the captured kicks" % (k + 1))
        assert g.update_result() == dict(done=1500, updated=1500, not_live=0, foreign=0, invalid=0, duplicate=0)
    cap.close()
    # refused under capture: a new mass or age (by id and by export order), and a scratch that would have to grow
    big_ids = torch.zeros(50000, dtype=torch.int32, device=DEV)
    big_vel = torch.zeros((50000, 4), dtype=torch.float32, device=DEV)
    with captured(g) as cap:
        rcs = [raw(g, MASS, 2000, ids, None, w), raw(g, AGE | ORDER, 2000, None, vel4), raw(g, VEL | MASS | ADD, 2000, ids, vel4, w),
               raw(g, VEL, 50000, big_ids, big_vel)]
        msg = lib.psamd_last_error(g.h)
    assert rcs == [ERR_STATE] * 4 and b"captured" in msg and b"grow" in msg, (rcs, msg)
    assert cap.nodes() == 0
    cap.close()
    assert_same_particles(g.download_particles(), want, "after the refused captures")
    assert raw(g, VEL, 50000, big_ids, big_vel) == OK           # outside a capture the scratch grows
    g.step(2)
    g.synchronize()
    g.close()


# ---- 6: slabs ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3])
def test_slabs(world):
    n = 30000
    xyz = cloud(n, 600 + world)
    rng = np.random.default_rng(world)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    fert = rng.uniform(3.0, 12.0, n).astype(np.float32)

    def make(**over):
        s = ps.ParticleSystem(ps.default_config(flags=ps.FLAG_EXPLOSIONS, seed=60 + world, **over))
        s.fill_particles(xyz, age=age, fert_age=fert)
        return s
    ranks = [make(rank=r, world=world) for r in range(world)]
    one = make()
    plans = [s.slab_plan() for s in ranks]
    assert any(pl.lentin_lo < pl.lentin_hi or pl.lentout_lo < pl.lentout_hi for pl in plans), "default cuts: layers are lent"
    cont = one.sizes.container_size

    def same_as_one(what):
        union = merge_owned([s.download_particles() for s in ranks], plans)
        assert_same_particles(union, one.download_particles(), what + ": union vs one context")
        qs = [s.download_queues() for s in ranks]
        qi1, q1 = one.download_queues()
        assert merge_owned([x[0] for x in qs], plans, "records").tobytes() == qi1.tobytes(), what + ": QUEUE_INFO records"
        assert np.array_equal(merge_owned([x[1] for x in qs], plans), q1), what + ": queues"

    def by_id_everywhere(fields, ids, vel4, w, fert_new, r1, out1, what):
        """every rank is given all entries: one answer 0 per live id, the others 2; the results add up to the one context's"""
        valid = (ids >= 0) & (ids < cont)
        total = dict.fromkeys(U.RESULT_KEYS, 0)
        answered = np.zeros(len(ids), int)
        for rank, (s, pl) in enumerate(zip(ranks, plans)):
            owned = np.zeros(cont, bool)
            for t in range(4):
                owned[pl.slot_lo[t]:pl.slot_hi[t]] = True
            mine = valid & owned[np.where(valid, ids, 0)]
            r, out = update(s, fields, ids, vel4, w, fert_new)
            assert np.array_equal(out[mine], out1[mine]) and (out[valid & ~mine] == U.FOREIGN).all() and (out[~valid] == U.INVALID).all(), (what, rank)
            answered += out == U.UPDATED
            for k in total:
                total[k] += r[k]
        assert np.array_equal(answered == 1, out1 == U.UPDATED) and answered.max() == 1, what
        assert total == ps.merge_update([dict(r1, done=world * len(ids), invalid=world * r1["invalid"],
                                              foreign=(world - 1) * int(valid.sum()))]), (what, total, r1)

    for _ in range(2):
        step_local(ranks)
    one.step(2)
    cell = one.download_particles()["cell"]
    live, free = np.nonzero(cell >= 0)[0], np.nonzero(cell < 0)[0]
    ids = np.concatenate([rng.permutation(live)[:8000], rng.choice(live, 1000), rng.choice(free, 500), [-3, cont, cont + 7]]).astype(np.int32)
    rng.shuffle(ids)
    vel4, w, fert_new = entries(len(ids), 70 + world)
    vel4[:, :3] *= 0.2
    # between frames, all four words
    r1, out1 = update(one, VEL | AGE | MASS | FERT, ids, vel4, w, fert_new)
    assert r1["updated"] >= 8000 and r1["duplicate"] > 0 and r1["invalid"] == 3
    by_id_everywhere(VEL | AGE | MASS | FERT, ids, vel4, w, fert_new, r1, out1, "world %d between frames" % world)
    same_as_one("world %d by id between frames" % world)
    # by export order a rank's entries are its own export's
    e1 = one.export_live(ps.EXPORT_ID)["id"].cpu().numpy()
    table = entries(cont, 80 + world)[0]
    assert update(one, VEL, None, np.ascontiguousarray(table[e1]))[0]["updated"] == len(e1)
    for s in ranks:
        er = s.export_live(ps.EXPORT_ID)["id"].cpu().numpy()
        assert update(s, VEL, None, np.ascontiguousarray(table[er]))[0]["updated"] == len(er)
    same_as_one("world %d by export order" % world)

    # inside the step: behind the pair stage the kick is the one this step integrates
    def kick(rs):
        by_id_everywhere(VEL | ADD | FERT, ids, vel4, w, fert_new, r2, out2, "world %d in ST_SLAB_PAIRS" % world)
    one.init_iframe(); one.build_grid(); one.calc_forces_pairs()
    r2, out2 = update(one, VEL | ADD | FERT, ids, vel4, w, fert_new)
    one.calc_forces_apply()
    step_local(ranks, after_pairs=kick)
    same_as_one("world %d, the step of the kick" % world)
    for k in range(2):
        step_local(ranks)
        one.step(1)
        same_as_one("world %d, step %d after the kick" % (world, k + 1))

    # between slab_apply and slab_finish every form is refused, and the step completes
    d_ids, d_vel, d_w = dev(ids), dev(vel4), dev(w)

    def refused(rs):
        for s in rs:
            rcs = [raw(s, VEL, len(ids), d_ids, d_vel), raw(s, VEL | ADD, len(ids), d_ids, d_vel), raw(s, FERT | ORDER, 100, None, None, None, d_w),
                   raw(s, MASS, len(ids), d_ids, None, d_w), raw(s, AGE | ORDER, 100, None, d_vel), raw(s, VEL, 0)]
            assert rcs == [ERR_STATE] * 6 and b"slab_apply" in s.lib.psamd_last_error(s.h), rcs
    torch.cuda.synchronize()
    step_local(ranks, after_apply=refused)
    one.step(1)
    same_as_one("world %d, the step with the refused updates" % world)
    for s in ranks + [one]:
        s.close()


# ---- 7: arguments ------------------------------------------------------------------------------------------------------------------------

def test_arguments():
    a, b = start(seed=18), start(seed=18)
    a.step(1)
    b.step(1)
    ids = torch.arange(0, 1001, dtype=torch.int32, device=DEV)
    vel4 = torch.ones((1001, 4), dtype=torch.float32, device=DEV)
    w = torch.ones(1001, dtype=torch.float32, device=DEV)
    out = torch.zeros(1001, dtype=torch.int32, device=DEV)
    res = torch.zeros(8, dtype=torch.int64, device=DEV)
    cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    lib = b.lib

    def spec(**over):
        s = ps.Update(fields=VEL, max_count=1000, ids=ids.data_ptr(), vel4=vel4.data_ptr(), w=w.data_ptr(), fert_age=w.data_ptr(),
                      outcome_dev=out.data_ptr())
        for k, v in over.items():
            setattr(s, k, v)
        return s
    assert lib.psamd_update(None, C.byref(spec())) == ERR_INVALID_ARG
    assert lib.psamd_update(b.h, None) == ERR_INVALID_ARG
    assert lib.psamd_update_result_get(b.h, None) == ERR_INVALID_ARG
    for bad in (spec(fields=0), spec(fields=ADD), spec(fields=ORDER, ids=None), spec(fields=ADD | MASS), spec(fields=VEL | 0x10), spec(fields=VEL | 0x400),
                spec(fields=VEL | 0x80000000), spec(reserved=1), spec(max_count=-1), spec(max_count=1 << 31),
                spec(ids=None), spec(fields=VEL | ORDER), spec(vel4=None), spec(fields=AGE, vel4=None), spec(fields=MASS, w=None),
                spec(fields=FERT, fert_age=None), spec(fields=VEL | ORDER, ids=None, vel4=None),
                spec(ids=ids.data_ptr() + 2), spec(vel4=vel4.data_ptr() + 8), spec(fields=MASS, w=w.data_ptr() + 2),
                spec(fields=FERT, fert_age=w.data_ptr() + 2), spec(outcome_dev=out.data_ptr() + 2),
                spec(count_dev=cnt.data_ptr() + 4), spec(result_dev=res.data_ptr() + 4)):
        assert lib.psamd_update(b.h, C.byref(bad)) == ERR_INVALID_ARG, [(n, getattr(bad, n)) for n, _ in bad._fields_]
    b.synchronize()
    assert state(a)[0].tobytes() == state(b)[0].tobytes(), "after the refused calls"
    # arrays the fields do not name are not looked at
    assert lib.psamd_update(b.h, C.byref(spec(fields=MASS, vel4=None, fert_age=None))) == OK
    assert lib.psamd_update(a.h, C.byref(spec(fields=MASS, vel4=0x10, fert_age=0x4))) == OK
    assert a.update_result() == b.update_result() and b.update_result()["done"] == 1000
    # max_count == 0: a zero record, nothing else
    res.fill_(-1)
    torch.cuda.synchronize()
    assert lib.psamd_update(b.h, C.byref(spec(max_count=0, ids=None, vel4=None, outcome_dev=None, result_dev=res.data_ptr()))) == OK
    assert b.update_result() == dict.fromkeys(U.RESULT_KEYS, 0)
    assert res[:6].cpu().tolist() == [0] * 6 and res[6:].cpu().tolist() == [-1, -1]
    assert lib.psamd_update(b.h, C.byref(spec(fields=VEL | ORDER, max_count=0, ids=None, vel4=None))) == OK
    assert b.update_result() == dict.fromkeys(U.RESULT_KEYS, 0)
    # result_dev gets the record the context keeps
    assert lib.psamd_update(b.h, C.byref(spec(fields=MASS, result_dev=res.data_ptr()))) == OK
    r = b.update_result()
    assert res[:6].cpu().tolist() == [r[k] for k in U.RESULT_KEYS] and r["done"] == 1000 and r["updated"] > 0
    assert lib.psamd_update(a.h, C.byref(spec(fields=MASS))) == OK
    assert state(a)[0].tobytes() == state(b)[0].tobytes()
    for g in (a, b):
        g.close()


def test_a_wedged_context_is_refused(monkeypatch):
    """A context wedges when a step's scalars have not arrived within PSAMD_WAIT_LIMIT_S while its stream is still busy.  Here
    the limit is the library's floor of 0.05 s and the stream is busy with about 0.2 s of torch's spin kernel in front of the
    step: nothing hangs, the work drains, and the context refuses every later call as the header says."""
    monkeypatch.setenv("PSAMD_WAIT_LIMIT_S", "0.05")
    g = start(seed=19, run_ahead=0)
    g.step(1)
    live = np.nonzero(g.download_particles()["cell"] >= 0)[0]
    ids, vel4 = dev(live[:1000].astype(np.int32)), dev(entries(1000, 19)[0])
    ext = torch.cuda.ExternalStream(g.stream(), device=DEV)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(ext):
        torch.cuda._sleep(1000)                     # (the kernel's first launch)
        e0.record()
        torch.cuda._sleep(20_000_000)               # how long the spin kernel's cycle is
        e1.record()
    e1.synchronize()
    per_ms = 20_000_000 / e0.elapsed_time(e1)
    with torch.cuda.stream(ext):
        torch.cuda._sleep(int(200 * per_ms))
    lib = g.lib
    assert lib.psamd_step(g.h, 1) == ERR_STATE and b"stopped answering" in lib.psamd_last_error(g.h)
    before = g.download_particles()                 # (waits until the stream has drained: the step itself ran)
    for fields, i in ((VEL, ids), (VEL | ADD, ids), (VEL | ORDER, None), (MASS | ORDER, None)):
        assert raw(g, fields, 1000, i, vel4, ids) == ERR_STATE, hex(fields)        # (w: any aligned pointer, never read)
        assert b"stopped answering" in lib.psamd_last_error(g.h)
    assert raw(g, VEL, 0) == ERR_STATE
    assert lib.psamd_update_result_get(g.h, C.byref(ps.UpdateResult())) == ERR_STATE
    assert g.download_particles().tobytes() == before.tobytes()
    g.close()
