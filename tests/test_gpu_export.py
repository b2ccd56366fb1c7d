"""Getting frames out (psamd_export_live / psamd_download_live / psamd_live_stats_get, export.hip): the live particles
as compact arrays in slot order and their statistics.  What must hold: every field equals, bit for bit, the records of
download_particles() filtered by the live predicate (0 <= cell < num_cells) at the same point of the stream; the count
and capacity rules; statistics that agree with numpy in fp64 and repeat to the bit; slabs whose union is the single
context's export; stream order without a host sync, also inside a captured graph; the C++ driver's frames."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import particlesystem_amd as ps
from particlesystem_amd import _build as psbuild
from particlesystem_amd.slab import step_local
from service_harness import captured, host, start
from util import GOLDEN, O, SENTINEL, capacities, cloud, g2_cloud, ragged

pytestmark = pytest.mark.gpu

ALL = ps.EXPORT_ALL
SUMS = ("mass", "momentum", "kinetic", "mass_moment", "age_sum")


def sync(g):
    """wait for the context's stream (and nothing else)"""
    torch.cuda.ExternalStream(g.stream()).synchronize()


def live_records(p, num_cells):
    return p[(p["cell"] >= 0) & (p["cell"] < num_cells)]


def fields_of(rec):
    """the export's arrays as the records hold them"""
    return {"pos4": np.stack([rec["x"], rec["y"], rec["z"], rec["w"]], 1),
            "vel4": np.stack([rec["vx"], rec["vy"], rec["vz"], rec["age"]], 1),
            "acc4": np.stack([rec["ax"], rec["ay"], rec["az"], rec["fertility_age"]], 1),
            "id": rec["id"].astype(np.int32), "cell": rec["cell"].astype(np.int32)}


def same_bits(a, b, what):
    a, b = host(a), host(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.nonzero((a.view(np.uint32) if a.dtype == np.float32 else a) != (b.view(np.uint32) if b.dtype == np.float32 else b))[0]
    assert len(bad) == 0, "%s differs at %d entries, first %d: %r vs %r" % (what, len(bad), bad[0], a[bad[0]], b[bad[0]])


def check_export(got, rec, what, fields=ALL):
    assert got["count"] == len(rec), (what, got["count"], len(rec))
    want = fields_of(rec)
    for name, bit, _, _ in ps._EXPORT_FIELDS:
        if fields & bit:
            same_bits(got[name], want[name], "%s: %s" % (what, name))


def numpy_stats(rec):
    """fp64 statistics of downloaded records, with the library's definitions (include/psamd.h psamd_live_stats);
    also the sums of the terms' magnitudes, the scale of the rounding of a sum"""
    f = {k: rec[k].astype(np.float64) for k in ("x", "y", "z", "w", "vx", "vy", "vz", "age")}
    fin = np.ones(len(rec), bool)
    for k in ("x", "y", "z", "vx", "vy", "vz"):
        fin &= np.isfinite(f[k])
    f = {k: v[fin] for k, v in f.items()}
    w, v = f["w"], np.stack([f["vx"], f["vy"], f["vz"]], 1)
    xyz = np.stack([f["x"], f["y"], f["z"]], 1)
    terms = {"mass": w, "momentum": w[:, None] * v, "kinetic": 0.5 * w * (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]),
             "mass_moment": w[:, None] * xyz, "age_sum": f["age"]}
    s = {"live": len(rec), "nonfinite": int((~fin).sum())}
    scale = {}
    for k, t in terms.items():
        s[k] = t.sum(0)
        scale[k] = np.abs(t).sum(0)
    inf = np.float64(np.inf)
    s["lo"] = xyz.min(0) if len(xyz) else np.full(3, inf)
    s["hi"] = xyz.max(0) if len(xyz) else np.full(3, -inf)
    s["age_min"] = f["age"].min() if len(xyz) else inf
    s["age_max"] = f["age"].max() if len(xyz) else -inf
    return s, scale


def check_stats(got, rec, what):
    want, scale = numpy_stats(rec)
    for k in ("live", "nonfinite"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("lo", "hi", "age_min", "age_max"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k, got[k], want[k])
    for k in SUMS:
        err = np.abs(np.asarray(got[k]) - np.asarray(want[k]))
        assert np.all(err <= 1e-12 * np.asarray(scale[k]) + 1e-300), (what, k, got[k], want[k])


def check_all(g, what):
    """export_live and download_live against the filtered download, at this point of the stream"""
    rec = live_records(g.download_particles(), g.sizes.num_cells)
    got = g.export_live(ALL)
    check_export(got, rec, what + " (export_live)")
    check_stats(got["stats"], rec, what + " (stats)")
    check_export(g.download_live(ALL), rec, what + " (download_live)")
    return rec


@pytest.mark.parametrize("graphs,run_ahead", [(False, 0), (False, 1), (True, 0), (True, 1)])
def test_export_equals_the_filtered_download(graphs, run_ahead):
    g = start(graphs=graphs, run_ahead=run_ahead)
    check_all(g, "after the fill")
    g.step(1)
    check_all(g, "after 1 step")
    g.step(9)
    rec = check_all(g, "after 10 steps")
    c = g.counters
    assert c["births"] > 0 and c["relocations"] > 0, c
    assert len(rec) > 1000
    g.close()


def test_export_between_build_grid_and_calc_forces():
    g = start(seed=13)
    g.step(2)
    g.init_iframe()
    g.build_grid()
    check_all(g, "after build_grid")
    g.calc_forces()
    check_all(g, "after calc_forces")
    g.close()


def test_count_and_capacity():
    g = start(seed=14)
    g.step(3)
    rec = live_records(g.download_particles(), g.sizes.num_cells)
    n = g.live_count()
    assert n == len(rec) and g.export_live(0)["count"] == n and g.download_live(0)["count"] == n
    want = fields_of(rec)
    # a third of the count: exactly that prefix is written, the sentinel stays behind it, the full count is reported
    cap = n // 3
    dev = torch.device("cuda", 0)
    sentinel = -0x12345679
    arrs = {"pos4": torch.full((n, 4), sentinel, dtype=torch.int32, device=dev),
            "vel4": torch.full((n, 4), sentinel, dtype=torch.int32, device=dev),
            "acc4": torch.full((n, 4), sentinel, dtype=torch.int32, device=dev),
            "id": torch.full((n,), sentinel, dtype=torch.int32, device=dev),
            "cell": torch.full((n,), sentinel, dtype=torch.int32, device=dev)}
    count = torch.full((1,), -1, dtype=torch.int64, device=dev)
    stats = torch.zeros(C.sizeof(ps.LiveStats), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    spec = ps.Export(fields=ALL, capacity=cap, count_dev=count.data_ptr(), stats_dev=stats.data_ptr(),
                     **{k: t.data_ptr() for k, t in arrs.items()})
    assert g.lib.psamd_export_live(g.h, C.byref(spec)) == 0
    sync(g)
    assert count.item() == n
    for k, t in arrs.items():
        a = t.cpu().numpy()
        same_bits(a[:cap].view(np.float32) if k.endswith("4") else a[:cap], want[k][:cap], "capacity prefix " + k)
        assert (a[cap:] == sentinel).all(), k
    check_stats(ps.LiveStats.from_buffer_copy(stats.cpu().numpy().tobytes()).to_dict(), rec, "capacity n // 3")
    # the host variant with the same capacity
    got = g.download_live(ALL, capacity=cap)
    assert got["count"] == n and len(got["id"]) == cap
    for k in arrs:
        same_bits(got[k], want[k][:cap], "download_live capacity prefix " + k)
    # capacity 0 and no fields: the count and the statistics still arrive
    count.fill_(-1)
    stats.zero_()
    torch.cuda.synchronize()
    spec0 = ps.Export(fields=0, capacity=0, count_dev=count.data_ptr(), stats_dev=stats.data_ptr())
    assert g.lib.psamd_export_live(g.h, C.byref(spec0)) == 0
    sync(g)
    assert count.item() == n
    check_stats(ps.LiveStats.from_buffer_copy(stats.cpu().numpy().tobytes()).to_dict(), rec, "capacity 0")
    check_stats(g.live_stats(), rec, "live_stats")
    g.close()


def test_empty_system_and_invalid_arguments():
    g = ps.ParticleSystem(ps.default_config())
    got = g.export_live(ALL)
    assert got["count"] == 0 and all(len(got[k]) == 0 for k in ("pos4", "id"))
    s = g.live_stats()
    assert s["live"] == 0 and s["nonfinite"] == 0 and s["mass"] == 0.0
    assert (s["lo"] == np.inf).all() and (s["hi"] == -np.inf).all() and s["age_min"] == np.inf and s["age_max"] == -np.inf
    assert g.download_live(ps.EXPORT_POS)["count"] == 0
    lib, h = g.lib, g.h
    buf = torch.zeros((16, 4), dtype=torch.float32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    ok = dict(fields=ps.EXPORT_POS, capacity=16, pos4=buf.data_ptr(), count_dev=count.data_ptr())
    assert lib.psamd_export_live(h, C.byref(ps.Export(**ok))) == 0
    bad = [dict(ok, fields=0x20), dict(ok, fields=ps.EXPORT_POS | 0x100), dict(ok, capacity=-1), dict(ok, pos4=None),
           dict(ok, fields=ps.EXPORT_POS | ps.EXPORT_ID), dict(ok, reserved=1), dict(ok, pos4=buf.data_ptr() + 4)]
    for b in bad:
        assert lib.psamd_export_live(h, C.byref(ps.Export(**b))) == 1, b
    assert lib.psamd_export_live(None, C.byref(ps.Export(**ok))) == 1
    assert lib.psamd_export_live(h, None) == 1
    n = C.c_int64()
    host_pos = np.zeros((4, 4), np.float32)
    assert lib.psamd_download_live(h, ps.EXPORT_POS, host_pos.ctypes.data, None, None, None, None, 4, None) == 1
    assert lib.psamd_download_live(h, ps.EXPORT_ID, host_pos.ctypes.data, None, None, None, None, 4, C.byref(n)) == 1
    assert lib.psamd_download_live(h, 0x40, None, None, None, None, None, 4, C.byref(n)) == 1
    assert lib.psamd_download_live(None, 0, None, None, None, None, None, 0, C.byref(n)) == 1
    assert lib.psamd_live_stats_get(h, None) == 1 and lib.psamd_live_stats_get(None, C.byref(ps.LiveStats())) == 1
    torch.cuda.synchronize()
    g.close()


def test_statistics_repeat_to_the_bit_with_graphs_on_and_off():
    runs = []
    for graphs in (False, True):
        g = start(seed=15, graphs=graphs)
        g.step(6)
        rec = live_records(g.download_particles(), g.sizes.num_cells)
        a, b = ps.LiveStats(), ps.LiveStats()
        assert g.lib.psamd_live_stats_get(g.h, C.byref(a)) == 0 and g.lib.psamd_live_stats_get(g.h, C.byref(b)) == 0
        assert bytes(a) == bytes(b), "two calls on the same state"
        check_stats(a.to_dict(), rec, "graphs %s" % graphs)
        dev = g.export_live(ps.EXPORT_POS)["stats"]
        assert all(np.array_equal(np.asarray(dev[k]), np.asarray(a.to_dict()[k])) for k in dev), "export_live vs live_stats"
        runs.append(bytes(a))
        g.close()
    assert runs[0] == runs[1], "graphs on vs off"


def test_particles_whose_position_is_not_a_number_are_counted_and_left_out():
    """built as test_gpu_parity's not-a-number case: a kid and an adult with the velocity 0/0 among a dense crowd"""
    rng = np.random.default_rng(171)
    n = 1500
    corner = np.stack([rng.uniform(-39.9, -30.1, n), rng.uniform(30.1, 39.9, n), rng.uniform(30.1, 39.9, n)], axis=1).astype(np.float32)
    xyz = np.concatenate([corner, cloud(2000, 172)]).astype(np.float32)
    m = len(xyz)
    age = rng.uniform(2.0, 9.0, m).astype(np.float32)
    v = rng.uniform(-3, 3, (m, 3)).astype(np.float32)
    xyz[0] = (1.0, 2.0, 3.0); age[0] = 0.05; v[0] = np.nan
    xyz[1] = (-7.0, 4.0, -9.0); age[1] = 4.0; v[1] = np.nan
    g = ps.ParticleSystem(ps.default_config())
    g.fill_particles(xyz, age=age, fert_age=np.float32(1e6), vxyz=v)
    nan_positions = 0
    for k in range(5):
        if k:
            g.step(1)
        rec = check_all(g, "not-a-number particles, step %d" % k)
        s = g.live_stats()
        check_stats(s, rec, "not-a-number particles, step %d (live_stats)" % k)
        assert np.isfinite(s["mass"]) and np.isfinite(s["kinetic"]) and np.isfinite(s["lo"]).all() and np.isfinite(s["hi"]).all(), s
        assert s["nonfinite"] >= (2 if k == 0 else 0)
        nan_positions += int(np.isnan(rec["x"]).sum())
    assert nan_positions >= 1
    g.close()


@pytest.mark.parametrize("world", [2, 3])
def test_slab_union_equals_the_single_context(world):
    n = 60000
    xyz = cloud(n, 400 + world)
    rng = np.random.default_rng(world)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    fert = rng.uniform(3.0, 12.0, n).astype(np.float32)
    seed = 40 + world
    ranks = [ps.ParticleSystem(ps.default_config(rank=r, world=world, flags=ps.FLAG_EXPLOSIONS, seed=seed)) for r in range(world)]
    for s in ranks:
        s.fill_particles(xyz, age=age, fert_age=fert)
    one = ps.ParticleSystem(ps.default_config(flags=ps.FLAG_EXPLOSIONS, seed=seed))
    one.fill_particles(xyz, age=age, fert_age=fert)
    for _ in range(12):
        step_local(ranks)
    one.step(12)
    whole = one.export_live(ALL)
    rec = live_records(one.download_particles(), one.sizes.num_cells)
    check_export(whole, rec, "single context")
    parts = [s.export_live(ALL) for s in ranks]
    for p in parts:
        ids = host(p["id"])
        assert (np.diff(ids) > 0).all(), "a rank's export is in ascending global id"
    ids = np.concatenate([host(p["id"]) for p in parts])
    order = np.argsort(ids, kind="stable")
    for k in ("pos4", "vel4", "acc4", "id", "cell"):
        same_bits(np.concatenate([host(p[k]) for p in parts])[order], whole[k], "world %d union: %s" % (world, k))
    assert sum(p["count"] for p in parts) == whole["count"]
    merged = ps.merge_live_stats([p["stats"] for p in parts])
    check_stats(merged, rec, "world %d merged statistics" % world)
    for k in ("live", "nonfinite", "lo", "hi", "age_min", "age_max"):
        assert np.array_equal(np.asarray(merged[k]), np.asarray(whole["stats"][k])), k
    _, scale = numpy_stats(rec)
    for k in SUMS:
        assert np.all(np.abs(np.asarray(merged[k]) - np.asarray(whole["stats"][k])) <= 1e-12 * np.asarray(scale[k]) + 1e-300), k
    # the host variant, rank by rank
    got = [s.download_live(ps.EXPORT_ID | ps.EXPORT_POS) for s in ranks]
    ids = np.concatenate([x["id"] for x in got])
    order = np.argsort(ids)
    same_bits(np.concatenate([x["pos4"] for x in got])[order], whole["pos4"], "world %d download_live union" % world)
    for s in ranks + [one]:
        s.close()


def test_export_follows_the_step_in_stream_order_and_replays_from_a_graph():
    g, o = start(seed=16, graphs=True, run_ahead=1, oracle=True)
    cap = g.owned_slots()
    dev = torch.device("cuda", 0)
    pos = torch.empty((cap, 4), dtype=torch.float32, device=dev)
    ids = torch.empty((cap,), dtype=torch.int32, device=dev)
    count = torch.full((1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    spec = ps.Export(fields=ps.EXPORT_POS | ps.EXPORT_ID, capacity=cap, pos4=pos.data_ptr(), id=ids.data_ptr(),
                     count_dev=count.data_ptr())
    # step 5 and the export back to back: no synchronisation in between
    assert g.lib.psamd_step(g.h, 5) == 0
    assert g.lib.psamd_export_live(g.h, C.byref(spec)) == 0
    sync(g)
    o.step(5)
    want = o.particles[o.particles["cell"] >= 0]
    n = int(count.item())
    assert n == len(want)
    same_bits(pos[:n], fields_of(want)["pos4"], "step 5: positions")
    same_bits(ids[:n], fields_of(want)["id"], "step 5: ids")
    # the export alone, captured into a graph on the context's stream (two kernel nodes, one after the other)
    with captured(g) as cap:
        rc = g.lib.psamd_export_live(g.h, C.byref(spec))
    assert rc == 0
    g.step(1)
    count.fill_(-1)
    pos.fill_(0.0)
    torch.cuda.synchronize()
    cap.launch()
    got = g.download_live(ps.EXPORT_POS | ps.EXPORT_ID)
    n = int(count.item())
    assert n == got["count"]
    same_bits(pos[:n], got["pos4"], "graph replay after step 6: positions")
    same_bits(ids[:n], got["id"], "graph replay after step 6: ids")
    o.step(1)
    assert n == int((o.particles["cell"] >= 0).sum())
    cap.close()
    g.close(); o.close()


def digest(particles):
    """state_digest of host/ps_driver.cpp on a P_DATA_TYPE array"""
    w = np.ascontiguousarray(particles).view(np.uint32).reshape(-1, 18).copy()
    w[:, 5] &= 0x0000FFFF
    flat = w.reshape(-1).astype(np.uint64)
    k = np.arange(flat.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int((flat * (k % np.uint64(65521) + np.uint64(1))).sum(dtype=np.uint64))


def test_driver_writes_frames(tmp_path):
    xyz = g2_cloud()
    dt = 0.01
    o = O.System(dt=dt)
    o.fill(xyz, age=np.float32(40 * dt), fert_age=(1e6 + np.arange(len(xyz))).astype(np.float32))
    o.step(10)
    exe = psbuild.build_driver()
    out = subprocess.run([exe, "--cloud", os.path.join(GOLDEN, "g2_cloud_n4096_seed12345.f32"), "--iters", "10", "--dt", str(dt),
                          "--frames", str(tmp_path), "--frame-every", "5"], check=True, capture_output=True, text=True,
                         timeout=600).stdout
    assert sorted(os.listdir(tmp_path)) == ["frame_10.bin", "frame_5.bin"]
    raw = (tmp_path / "frame_10.bin").read_bytes()
    n = int(np.frombuffer(raw[:8], np.int64)[0])
    want = o.particles[o.particles["cell"] >= 0]
    assert n == len(want) and len(raw) == 8 + n * 20
    same_bits(np.frombuffer(raw[8:8 + 16 * n], np.float32).reshape(n, 4), fields_of(want)["pos4"], "frame 10: positions")
    same_bits(np.frombuffer(raw[8 + 16 * n:], np.int32), fields_of(want)["id"], "frame 10: ids")
    m = re.search(r"state-hash ([0-9a-f]{16}) live (\d+)", out)
    assert m and int(m.group(1), 16) == digest(o.particles) and int(m.group(2)) == len(want), out
    o.close()


# ---- a container that is no whole number of slot tiles ------------------------------------------------------------------
# The default container is 4096 * 514 slots.  This one has 125 segments of 144 slots = 18 000: four tiles of 4096 and one of
# 1616, whose slots are corner segments -- every cell of a uniform cloud fills some of them (util.ragged).

def test_ragged_last_tile():
    g, rec = ragged()
    got = g.export_live(ALL)
    assert int(got["id"].max()) == rec["id"].max()
    check_export(got, rec, "ragged last tile (export_live)")
    check_stats(got["stats"], rec, "ragged last tile (stats)")
    check_export(g.download_live(ALL), rec, "ragged last tile (download_live)")
    g.close()


def test_ragged_capacity_cuts():
    g, rec = ragged(seed=32)
    live, want = len(rec), fields_of(rec)
    dev = torch.device("cuda", 0)
    for cap in capacities(live):
        m = min(live, cap)
        arrs = {name: torch.full((cap + 1, width) if width > 1 else (cap + 1,), SENTINEL, dtype=torch.int32, device=dev)
                for name, _, width, _ in ps._EXPORT_FIELDS}
        count = torch.full((1,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        spec = ps.Export(fields=ALL, capacity=cap, count_dev=count.data_ptr(), **{k: t.data_ptr() for k, t in arrs.items()})
        assert g.lib.psamd_export_live(g.h, C.byref(spec)) == 0
        sync(g)
        assert count.item() == live, (cap, count.item(), live)
        for k, t in arrs.items():
            a = t.cpu().numpy()
            same_bits(a[:m].view(np.float32) if k.endswith("4") else a[:m], want[k][:m], "capacity %d: %s" % (cap, k))
            assert (a[m:] == SENTINEL).all(), "capacity %d: %s written past entry %d" % (cap, k, m)
        got = g.download_live(ALL, capacity=cap)
        assert got["count"] == live
        for k in arrs:
            same_bits(got[k], want[k][:m], "download_live capacity %d: %s" % (cap, k))
    g.close()
