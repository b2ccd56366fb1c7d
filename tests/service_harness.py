"""What the GPU tests of the on-stream services share (test_gpu_export.py, _inject, _remove, _update, _potential, _probe,
_deposit, and the slab and far-field tests that place a call inside a step): the header's status codes, a call captured into a
graph, arrays to and from the device, a context's state, the G2 start with its oracle, a batch put in two ways, a slab world
with its oracle.  The step cut open is particlesystem_amd.slab's (to_pairs, apply_stage, finish_stage, deliver, gather).

What belongs here: a helper that two or more test files need, word for word.  What does not: a service's own reference
(Ref, Frame, the *_model.py files), its clouds and grids, and anything that decides what one test asserts.  A test file takes
helpers from here or from util.py, never from another test file."""
import contextlib
import ctypes as C
import functools

import numpy as np
import torch

import particlesystem_amd as ps
from particlesystem_amd.slab import merge_owned
from util import O, assert_same_particles, cloud, explosion_rng, g2_cloud, oracle_cfg_from

# psamd_status (include/psamd.h)
OK, ERR_INVALID_ARG, ERR_OUTSIDE_BOX, ERR_QUEUE_EMPTY, ERR_STATE, ERR_UNSUPPORTED = 0, 1, 5, 6, 8, 9
DEV = torch.device("cuda", 0)


# ---- the HIP runtime, and a call captured into a graph -----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hip_runtime():
    """the HIP runtime torch loaded (the library is bound to the same copy)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64.so" in line:
            hip = C.CDLL(line.split()[-1])
            break
    else:
        raise RuntimeError("no HIP runtime in this process")
    vp = C.c_void_p
    for name, args in (("hipStreamBeginCapture", [vp, C.c_int]), ("hipStreamEndCapture", [vp, C.POINTER(vp)]),
                       ("hipGraphInstantiate", [C.POINTER(vp), vp, vp, vp, C.c_size_t]), ("hipGraphLaunch", [vp, vp]),
                       ("hipStreamSynchronize", [vp]), ("hipGraphExecDestroy", [vp]), ("hipGraphDestroy", [vp]),
                       ("hipGraphGetNodes", [vp, vp, C.POINTER(C.c_size_t)]), ("hipMemcpy", [vp, vp, C.c_size_t, C.c_int])):
        getattr(hip, name).restype = C.c_int
        getattr(hip, name).argtypes = args
    return hip


class _Capture:
    def __init__(self, stream):
        self.hip, self.stream, self.graph, self.exe = hip_runtime(), C.c_void_p(stream), C.c_void_p(), C.c_void_p()

    def launch(self):
        """one replay, waited for (the executable graph is made on the first)"""
        if not self.exe:
            assert self.hip.hipGraphInstantiate(C.byref(self.exe), self.graph, None, None, 0) == 0
        assert self.hip.hipGraphLaunch(self.exe, self.stream) == 0
        assert self.hip.hipStreamSynchronize(self.stream) == 0

    def nodes(self):
        n = C.c_size_t(99)
        assert self.hip.hipGraphGetNodes(self.graph, None, C.byref(n)) == 0
        return n.value

    def close(self):
        if self.exe:
            assert self.hip.hipGraphExecDestroy(self.exe) == 0
        assert self.hip.hipGraphDestroy(self.graph) == 0


@contextlib.contextmanager
def captured(g):
    """The calls made inside are captured on the context's stream (relaxed mode) and run nothing; the object given has
    launch(), nodes() and close().  The capture is ended whatever the body does, so a failing test leaves the stream usable; a
    refused call's status is taken inside and asserted after the block."""
    cap = _Capture(g.stream())
    torch.cuda.synchronize()
    assert cap.hip.hipStreamBeginCapture(cap.stream, 2) == 0       # hipStreamCaptureModeRelaxed
    done = False
    try:
        yield cap
        done = True
    finally:
        rc = cap.hip.hipStreamEndCapture(cap.stream, C.byref(cap.graph))
        if done:
            assert rc == 0, rc
        elif cap.graph:
            cap.hip.hipGraphDestroy(cap.graph)


# ---- arrays ------------------------------------------------------------------------------------------------------------------

def dev_read(ptr, count, dtype):
    """count entries of device memory at ptr"""
    out = np.zeros(count, dtype)
    assert hip_runtime().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2) == 0      # device to host
    return out


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def bits(a):
    return np.ascontiguousarray(host(a), np.float32).view(np.uint32)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- a context: its frame, its state ------------------------------------------------------------------------------------------

def open_frame(g):
    """a frame up to the window of the on-stream services, before the pair stage"""
    g.init_iframe()
    g.build_grid()


def kid_age(cfg):
    return cfg.life_steps * cfg.dt / 10.0           # KID_AGE = PARTICLE_LIFE / 10, PARTICLE_LIFE = 300 * DT (common.h:58-59)


def state(g):
    qi, q = g.download_queues()
    return g.download_particles(), qi, q


def same_state(a, b, what):
    pa, qia, qa = state(a)
    pb, qib, qb = state(b)
    assert_same_particles(pa, pb, what + ": particles")
    assert qia.tobytes() == qib.tobytes(), what + ": QUEUE_INFO records differ"
    assert np.array_equal(qa, qb), what + ": queues differ"


def start(seed=11, graphs=False, run_ahead=1, oracle=False, **over):
    """the G2 cloud with explosions: births, relocations and collisions from the first steps on"""
    xyz = g2_cloud()
    rng = np.random.default_rng(seed)
    age = rng.uniform(2.0, 9.0, len(xyz)).astype(np.float32)
    fert = rng.uniform(3.0, 12.0, len(xyz)).astype(np.float32)
    v = rng.uniform(-20, 20, xyz.shape).astype(np.float32)
    over.setdefault("flags", ps.FLAG_EXPLOSIONS)
    g = ps.ParticleSystem(ps.default_config(seed=seed, **over))
    g.set_graphs(graphs)
    g.set_run_ahead(run_ahead)
    g.fill_particles(xyz, age=age, fert_age=fert, vxyz=v)
    if not oracle:
        return g
    o = O.System(oracle_cfg_from(g.cfg))
    o.set_rng(explosion_rng(seed))
    ids = o.fill(xyz, age=age, fert_age=fert)
    p = o.particles
    p["vx"][ids], p["vy"][ids], p["vz"][ids] = v.T
    return g, o


# more queue records than a tile's counts have room for in LDS: queue_infos = (2 * chunk_factor + 1)^3 = 9261 > 8192, the tile
# counts live in the tile's row in global memory
MANY_RECORDS = dict(chunk_factor=10, chunk_dim=3, x_factor=2, max_particles_num=27000)


def many_records():
    g = ps.ParticleSystem(ps.default_config(**MANY_RECORDS))
    assert g.sizes.queue_info_size > 8192, g.sizes.queue_info_size
    return g


# ---- a batch of particles, put in by the host and by the device -----------------------------------------------------------------

def batch(g, n, seed):
    """n entries inside the box: pos4 (x, y, z, w), vel4 (vx, vy, vz, age), fert_age -- numpy float32"""
    rng = np.random.default_rng(seed)
    xyz = g.uniform_cloud(n, seed)
    pos4 = np.concatenate([xyz, rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)], 1)
    vel4 = np.concatenate([rng.uniform(-20, 20, (n, 3)), rng.uniform(0.0, 9.0, (n, 1))], 1).astype(np.float32)
    fert = rng.uniform(3.0, 12.0, n).astype(np.float32)
    return np.ascontiguousarray(pos4), np.ascontiguousarray(vel4), fert


def fill(g, pos4, vel4=None, fert=None):
    """psamd_fill_particles of the same entries: (status, done, ids[:done])"""
    n = len(pos4)
    xyz = np.ascontiguousarray(pos4[:, :3])
    w = np.ascontiguousarray(pos4[:, 3])
    vxyz = None if vel4 is None else np.ascontiguousarray(vel4[:, :3])
    age = None if vel4 is None else np.ascontiguousarray(vel4[:, 3])
    fert = None if fert is None else np.ascontiguousarray(fert)
    ids = np.full(max(n, 1), -7, np.int32)
    done = C.c_int64(-1)
    st = g.lib.psamd_fill_particles(g.h, n, ps._ptr(xyz), ps._ptr(vxyz), ps._ptr(w), ps._ptr(age), ps._ptr(fert),
                                    ps._ptr(ids), C.byref(done))
    return st, done.value, ids[:done.value]


def inject(g, pos4, vel4=None, fert=None, count=None):
    r = g.inject(dev(pos4), dev(vel4), dev(fert), count=count, ids=True)
    r["ids"] = r["ids"].cpu().numpy()
    return r


def same_as_fill(f, r, what, placed=None):
    st, done, ids = f
    assert (r["status"], r["done"]) == (st, done), (what, r, st, done)
    assert np.array_equal(r["ids"][:done], ids), what + ": ids"
    assert (r["ids"][done:] == -1).all(), what + ": ids at and after the stop"
    assert r["placed"] == (int((ids >= 0).sum()) if placed is None else placed), (what, r["placed"])


# ---- a slab world on one GPU, with the one-context oracle ------------------------------------------------------------------------

COUNTERS = ("deaths_age", "deaths_collision", "survives", "integrated", "relocations",
            "relocations_lost", "births", "births_failed", "cell_overflow_kills")


def make_world(world, xyz, age, fert, flags=0, cuts=None, **over):
    ranks = []
    for r in range(world):
        kw = dict(rank=r, world=world, flags=flags, **over)
        if cuts is not None:
            kw["cuts"] = cuts
        ranks.append(ps.ParticleSystem(ps.default_config(**kw)))
    o = O.System(oracle_cfg_from(ranks[0].cfg))
    ids_o = o.fill(xyz, age=age, fert_age=fert)
    ids = np.stack([g.fill_particles(xyz, age=age, fert_age=fert) for g in ranks])
    # every particle was placed by exactly one rank, in the slot the oracle gave it
    assert ((ids >= 0).sum(0) == 1).all()
    assert np.array_equal(ids.max(0), ids_o)
    return ranks, o


def compare_world(ranks, o, what):
    plans = [g.slab_plan() for g in ranks]
    p = merge_owned([g.download_particles() for g in ranks], plans)
    assert_same_particles(p, o.particles, what)
    qs = [g.download_queues() for g in ranks]
    qi = merge_owned([q[0] for q in qs], plans, "records")
    q = merge_owned([q[1] for q in qs], plans)
    assert qi.tobytes() == o.queue_info.tobytes(), what + ": QUEUE_INFO differs"
    assert np.array_equal(q, o.queue), what + ": queue array differs"
    cs = [g.counters for g in ranks]
    for k in COUNTERS:
        assert sum(c[k] for c in cs) == o.counters[k], (what, k, [c[k] for c in cs], o.counters[k])
    return cs


def slab_inputs(n, seed):
    """(xyz, age, v) of the field services' slab worlds: one particle in seven a kid"""
    rng = np.random.default_rng(seed)
    return cloud(n, seed), rng.uniform(0.2, 9.0, n).astype(np.float32), cloud(n, seed + 1, 20.0)
