"""The CPU oracle against the reference's own L4 code on seeded random inputs.  The reference's answers for exactly
these inputs are stored in tests/golden/ref_vs_oracle.npz (made by tests/golden/make_golden.py --vs-oracle with
oracle/_ref/libref_l4.so), so every test runs on any machine; where that library was built (oracle/Makefile, only
where the reference's sources are) the reference is also run live and must give the stored answers bit for bit."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle_py as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vs_oracle.npz")
PAIR_SEEDS = (1, 2, 3)
NAN, INF = float("nan"), float("inf")
SETPOS_ODD_CASES = [(NAN, NAN, NAN), (NAN, 1.0, -2.0), (3.0, NAN, 7.0), (1.0, 2.0, NAN), (INF, 0.0, 0.0), (0.0, -INF, 0.0), (1e30, -1e30, 5.0)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _blank(n):
    p = np.zeros(n, dtype=O.P_DTYPE)
    for f in ("cell", "chunk", "seg_type", "seg_tid"):
        p[f] = -1
    return p


def fields(p):
    """particle records field by field (their two pad bytes are not stored)"""
    return {f: np.ascontiguousarray(p[f]) for f in O.P_DTYPE.names}


def records(stored):
    """particle records from their stored fields, pad bytes zero as in _blank's (a copy of a record array would leave
    them undefined)"""
    p = np.zeros(len(stored["id"]), dtype=O.P_DTYPE)
    for f in O.P_DTYPE.names:
        p[f] = stored[f]
    return p


@functools.lru_cache(maxsize=None)
def _stored():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def reference(case, live):
    """The reference's answers for `case`: the stored ones -- and, where the reference library was built, what `live()`
    (the reference run now on the same inputs) returns, which must be the same bytes."""
    want = {k[len(case) + 2:]: v for k, v in _stored().items() if k.startswith(case + "__")}
    assert want, "no stored answers for " + case
    if O.have_ref():
        got = live()
        assert set(got) == set(want), case
        for k, v in got.items():
            assert np.asarray(v).dtype == want[k].dtype and np.asarray(v).tobytes() == want[k].tobytes(), (case, k)
    return want


# ---- the inputs, and the reference run on them (make_golden.py --vs-oracle stores what these return) ----------------

def pairs_inputs(seed):
    rng = np.random.default_rng(seed)
    d = O.derive(O.default_config())
    n = 20000
    bi, bj = _blank(n), np.zeros(n, dtype=O.T_DTYPE)
    bi["id"] = rng.integers(0, d.container_size, n)
    bj["id"] = rng.integers(0, d.container_size, n)
    for f in ("x", "y", "z"):
        bi[f] = rng.uniform(-40, 40, n).astype(np.float32)
        bj[f] = (bi[f] + rng.normal(scale=rng.choice([0.2, 3.0, 10.0]), size=n)).astype(np.float32)
    bi["age"] = rng.uniform(0, 16, n).astype(np.float32)
    bj["age"] = rng.uniform(0, 16, n).astype(np.float32)
    bj["w"] = rng.uniform(0, 100, n).astype(np.float32)
    a0 = rng.normal(size=(n, 3)).astype(np.float32)
    return bi, bj, a0


def pairs_ref(seed):
    bi, bj, a = pairs_inputs(seed)
    R = O.ref()
    f = np.zeros(len(bi), np.int32)
    R.ref_body_body_interaction(len(bi), bi.ctypes.data, bj.ctypes.data, a.ctypes.data)
    R.ref_body_body_collision(len(bi), bi.ctypes.data, bj.ctypes.data, f.ctypes.data)
    return {"a": a, "f": f}


def set_pos_inputs():
    rng = np.random.default_rng(7)
    n = 20000
    pos = rng.uniform(-130, 130, (n, 3)).astype(np.float32)
    a = _blank(n)
    a["seg_type"] = rng.choice([-1, 1, 2, 4, 8], n)
    a["seg_tid"] = rng.integers(-1, 64, n)
    return a, pos


def set_pos_ref():
    a, pos = set_pos_inputs()
    for k in range(len(a)):
        O.ref().ref_set_pos_x(a[k:k + 1].ctypes.data, *map(float, pos[k]))
    return fields(a)


def set_pos_odd_inputs():
    a = _blank(len(SETPOS_ODD_CASES))
    a["seg_type"] = 1
    a["seg_tid"] = 0
    return a


def set_pos_odd_ref():
    a = set_pos_odd_inputs()
    for k, pos in enumerate(SETPOS_ODD_CASES):
        O.ref().ref_set_pos_x(a[k:k + 1].ctypes.data, *pos)
    return fields(a)


def gather_inputs():
    """an oracle system over a real cell grid, and the cells to gather around"""
    rng = np.random.default_rng(11)
    s = O.System()
    xyz = rng.uniform(-40, 40, (20000, 3)).astype(np.float32)
    s.fill(xyz, age=2.0, fert_age=1e6)
    s.init_iframe()
    s.build_grid()
    cells = rng.integers(0, s.d.num_cells, 200)
    return s, cells


def gather_ref():
    s, cells = gather_inputs()
    buf = np.zeros(s.d.max_neib_particles, np.int32)
    counts, lists = [], []
    for cell in cells:
        n = O.ref().ref_fill_particles(int(cell), s.cellgrid.ctypes.data, buf.ctypes.data, len(buf))
        counts.append(n)
        lists.append(buf[:n].copy())
    s.close()
    return {"counts": np.array(counts, np.int32), "lists": np.concatenate(lists).astype(np.int32)}


def helpers_inputs():
    rng = np.random.default_rng(5)
    return rng.integers(0, 255, 72 * 4, dtype=np.uint8)


def helpers_ref():
    a = helpers_inputs().view(O.P_DTYPE)
    R = O.ref()
    R.ref_reset_particle(a[0:1].ctypes.data)
    R.ref_survive_particle(a[1:2].ctypes.data)
    return {"bytes": a.view(np.uint8).copy()}


def reference_answers():
    """every case's reference answers, run now (make_golden.py --vs-oracle)"""
    out = {}
    cases = [("pairs%d" % s, functools.partial(pairs_ref, s)) for s in PAIR_SEEDS] + [
        ("set_pos", set_pos_ref), ("set_pos_odd", set_pos_odd_ref), ("gather", gather_ref), ("helpers", helpers_ref)]
    for case, fn in cases:
        for k, v in fn().items():
            out[case + "__" + k] = v
    return out


# ---- the tests ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", PAIR_SEEDS)
def test_pairs_random(seed):
    c = O.default_config()
    d = O.derive(c)
    L = O.lib()
    bi, bj, a_me = pairs_inputs(seed)
    n = len(bi)
    f_me = np.zeros(n, np.int32)
    for k in range(n):
        L.pso_body_body_interaction(C.byref(c), C.byref(d), bi[k:k + 1].ctypes.data,
                                    bj[k:k + 1].ctypes.data, a_me[k:k + 1].ctypes.data)
        f_me[k] = L.pso_body_body_collision(C.byref(c), C.byref(d), bi[k:k + 1].ctypes.data,
                                            bj[k:k + 1].ctypes.data)
    ref = reference("pairs%d" % seed, functools.partial(pairs_ref, seed))
    assert np.array_equal(bits(a_me), bits(ref["a"]))
    assert np.array_equal(f_me, ref["f"])


def test_set_pos_random():
    c = O.default_config()
    d = O.derive(c)
    L = O.lib()
    b, pos = set_pos_inputs()
    for k in range(len(b)):
        L.pso_set_pos_x(C.byref(c), C.byref(d), b[k:k + 1].ctypes.data, *map(float, pos[k]))
    a = records(reference("set_pos", set_pos_ref))
    assert a.tobytes() == b.tobytes()


def test_set_pos_of_what_is_no_number():
    """A position that is not a number (a child born with the direction (0, 0, 0) has one a step later): the
    reference's set_pos_t converts floor(NaN) + G/2 to int -- INT_MIN on this host's cvttsd2si -- and its wrap loop
    walks that to cell index 0 on each axis of the default 16^3 grid (2^31 is a multiple of 16).  The oracle, the
    reference's compiled code and, through them, the kernels' conversion (k_apply) agree; so do +-inf and values far
    outside the box."""
    c = O.default_config()
    d = O.derive(c)
    L = O.lib()
    b = set_pos_odd_inputs()
    for k, pos in enumerate(SETPOS_ODD_CASES):
        L.pso_set_pos_x(C.byref(c), C.byref(d), b[k:k + 1].ctypes.data, *pos)
    a = records(reference("set_pos_odd", set_pos_odd_ref))
    for f in ("cell", "chunk", "seg_type", "seg_tid", "seg_fault"):
        assert np.array_equal(a[f], b[f]), (f, a[f], b[f])
    assert np.array_equal(bits(np.stack([a["x"], a["y"], a["z"]])), bits(np.stack([b["x"], b["y"], b["z"]])))
    assert a["cell"][0] == 0 and (a["cell"] >= 0).all() and (a["cell"] < 4096).all()


def test_neighbour_gather_matches_reference():
    """fill_cells + fill_particles over a real cell grid == the oracle's gather order."""
    s, cells = gather_inputs()
    ref = reference("gather", gather_ref)
    cg = s.cellgrid
    out27 = (C.c_int * 27)()
    start = np.concatenate([[0], np.cumsum(ref["counts"])])
    assert len(ref["counts"]) == len(cells)
    for j, cell in enumerate(cells):
        m = O.lib().pso_fill_cells(C.byref(s.d), int(cell), out27)
        mine = np.concatenate([cg[out27[i], 1:1 + cg[out27[i], 0]] for i in range(m)] or [np.zeros(0, np.int32)])
        n = int(ref["counts"][j])
        assert n == len(mine)
        assert np.array_equal(ref["lists"][start[j]:start[j] + n], mine)
    s.close()


def test_particle_state_helpers():
    L = O.lib()
    b = helpers_inputs().view(O.P_DTYPE)
    L.pso_reset_particle(b[0:1].ctypes.data)
    L.pso_survive_particle(b[1:2].ctypes.data)
    assert reference("helpers", helpers_ref)["bytes"].tobytes() == b.tobytes()
