"""Taking particles out without a GPU: the remove structs of include/psamd.h (psamd_remove_spec, psamd_remove_result),
their ctypes mirror and the cross-compiled library agree; and the closed form psamd_remove's kernels use
(tests/remove_model.py) equals the oracle's serial get_id_info + reset_particle + q_insert, byte for byte, over random
and crafted queue states."""
import ctypes
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import particlesystem_amd as ps
import remove_model as M
from util import O, cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {"psamd_remove_spec": ps.Remove, "psamd_remove_result": ps.RemoveResult}


def c_layout(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "psamd.h"', "int main(void) {"]
    for cname, py in STRUCTS.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in py._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
    lines.append('printf("flags %u %u\\n", PSAMD_REMOVE_BOX, PSAMD_REMOVE_OUTSIDE);')
    # the entry points have the signatures the mirror binds
    lines.append("int (*f)(psamd_ctx *, const psamd_remove_spec *) = psamd_remove; (void)f;")
    lines.append("int (*g)(psamd_ctx *, psamd_remove_result *) = psamd_remove_result_get; (void)g;")
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-c", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "layout_c.o")], check=True)      # the header is C as well as C++
    subprocess.run(["g++", "-x", "c++", "-std=c++17", "-Wall", "-Werror", "-c", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "layout.o")], check=True)
    subprocess.run(["g++", str(tmp_path / "layout.o"), "-L" + os.path.dirname(ps.LIB_PATH), "-lpsamd",
                    "-Wl,-rpath," + os.path.dirname(ps.LIB_PATH), "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {tuple(l.split()[:2]): int(l.split()[2]) for l in out.splitlines()}


def test_remove_structs_match_the_ctypes_mirror(tmp_path):
    ps.build()
    got = c_layout(tmp_path)
    for cname, py in STRUCTS.items():
        assert got[(cname, "sizeof")] == ctypes.sizeof(py), cname
        for field, _ in py._fields_:
            assert got[(cname, field)] == getattr(py, field).offset, (cname, field)
    assert got[("psamd_remove_result", "sizeof")] == 48 and got[("psamd_remove_spec", "sizeof")] == 72
    assert [n for n, _ in ps.RemoveResult._fields_] == list(M.RESULT_KEYS)
    assert (got[("flags", str(ps.REMOVE_BOX))], ps.REMOVE_BOX, ps.REMOVE_OUTSIDE) == (2, 1, 2)


def test_the_mirror_binds_both_entry_points_and_the_abi_is_still_8():
    text = open(os.path.join(ROOT, "include", "psamd.h")).read()
    assert int(re.search(r"#define PSAMD_ABI_VERSION (\d+)", text).group(1)) == 8 == ps.ABI_VERSION
    names = [n for n, _, _ in ps.ABI]
    assert "psamd_remove" in names and "psamd_remove_result_get" in names
    ps.build()
    lib = ps.load()
    assert lib.psamd_abi_version() == 8
    assert lib.psamd_remove(None, None) == 1 and lib.psamd_remove_result_get(None, None) == 1     # PSAMD_ERR_INVALID_ARG


def filled_oracle(seed, n=1500):
    o = O.System(O.default_config(max_particles_num=4096))
    rng = np.random.default_rng(seed)
    o.fill(cloud(n, seed), age=rng.uniform(2.0, 9.0, n).astype(np.float32), fert_age=rng.uniform(3.0, 12.0, n).astype(np.float32))
    return o, rng


def q_remove(o, rec):
    qi = o.queue_info
    seg = (C.c_int * 2)()
    o.L.pso_get_id_info(C.byref(o.d), int(qi["rloc"][rec]), seg)
    assert o.L.pso_get_info_rloc(C.byref(o.d), seg[0], seg[1]) == rec
    return o.L.pso_q_remove(qi.ctypes.data, o.queue.ctypes.data, C.byref(o.d), seg[0], seg[1])


def q_insert(o, rec, x):
    qi = o.queue_info
    seg = (C.c_int * 2)()
    o.L.pso_get_id_info(C.byref(o.d), int(qi["rloc"][rec]), seg)
    o.L.pso_q_insert(qi.ctypes.data, o.queue.ctypes.data, C.byref(o.d), seg[0], seg[1], int(x))


def make_live(o, slot):
    p = o.particles
    p["cell"][slot] = 0
    p["x"][slot] = 1.5
    p["age"][slot] = 3.0


def churn(o, rng):
    """Queue states as steps leave them, and the corners: random q_remove / q_insert rounds; some records emptied to
    (-1, -1, 0); some filled to seg_size; some with rear about to wrap.  Slots a queue handed out are made live (so that
    every record keeps queue entries == free slots, except the full ones, whose live slots stand for the foreign slots the
    cell-overflow rule frees into a record)."""
    qi, p = o.queue_info, o.particles
    nrec = len(qi)
    kinds = {"empty": [], "wrap": [], "full": []}
    for rec in range(nrec):
        mode = rng.integers(0, 6)
        seg = int(qi["seg_size"][rec])
        if mode == 0:                                         # emptied: front = rear = -1
            while qi["count"][rec] > 0:
                make_live(o, q_remove(o, rec))
            assert (qi["front"][rec], qi["rear"][rec]) == (-1, -1)
            kinds["empty"].append(rec)
        elif mode == 1:                                       # rear at the last position of the segment
            guard = 0
            while qi["rear"][rec] != qi["rloc"][rec] + seg - 1 and guard < 4 * seg:
                s = q_remove(o, rec)
                if s >= 0:
                    q_insert(o, rec, s)
                guard += 1
            for _ in range(int(rng.integers(1, 6))):          # room in front of it
                s = q_remove(o, rec)
                if s >= 0:
                    make_live(o, s)
            if qi["count"][rec] > 0 and qi["rear"][rec] == qi["rloc"][rec] + seg - 1:
                kinds["wrap"].append(rec)
        elif mode == 2:                                       # full while some of its slots are live
            k = 0
            while qi["count"][rec] < seg:
                q_insert(o, rec, int(qi["rloc"][rec]) + k % seg)
                k += 1
            kinds["full"].append(rec)
        else:                                                 # a few rounds of traffic
            for _ in range(int(rng.integers(0, 12))):
                if rng.integers(0, 2) and qi["count"][rec] > 0:
                    make_live(o, q_remove(o, rec))
                else:
                    lo = int(qi["rloc"][rec])
                    live = lo + np.nonzero(p["cell"][lo:lo + seg] >= 0)[0]
                    if len(live):
                        s = int(rng.choice(live))
                        o.L.pso_reset_particle(p.ctypes.data + 72 * s)
                        q_insert(o, rec, s)
    return kinds


def id_list(o, rng, m):
    """live ids, free slots, invalid ids, duplicates close by and far apart, runs of one record in descending order"""
    cont = o.d.container_size
    p, qi = o.particles, o.queue_info
    live = np.nonzero(p["cell"] >= 0)[0]
    ids = np.concatenate([rng.choice(live, m), rng.integers(0, cont, m // 4), rng.integers(-50, 0, 8),
                          rng.integers(cont, cont + 50, 8), [np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1, cont]])
    rng.shuffle(ids)
    rec = int(rng.integers(0, len(qi)))
    lo, seg = int(qi["rloc"][rec]), int(qi["seg_size"][rec])
    run = np.arange(lo + seg - 1, lo - 1, -1)
    ids = np.concatenate([ids[:m // 2], run, ids[m // 2:], ids[:40], run[::3]])
    return ids.astype(np.int32)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_the_closed_form_equals_the_serial_definition(seed):
    o, rng = filled_oracle(seed)
    kinds = churn(o, rng)
    assert all(len(v) > 0 for v in kinds.values()), kinds
    for rec in kinds["full"] + kinds["wrap"] + kinds["empty"]:         # every corner gets removals
        lo, seg = int(o.queue_info["rloc"][rec]), int(o.queue_info["seg_size"][rec])
        for s in range(lo, lo + min(seg, 5)):
            make_live(o, s)
    ids = id_list(o, rng, 3000)
    for rec in kinds["full"] + kinds["wrap"] + kinds["empty"]:
        lo = int(o.queue_info["rloc"][rec])
        ids = np.concatenate([ids, np.arange(lo, lo + 5, dtype=np.int32)[::-1]])
    owned = None
    if seed == 4:                                                       # a slab's view: some slot ranges are foreign
        owned = np.ones(o.d.container_size, bool)
        owned[o.d.container_size // 3: o.d.container_size // 2] = False
    p, qi, q, outcome, result = M.closed_form(o.d, o.d.num_cells, o.particles, o.queue_info, o.queue, ids, owned)
    s_outcome, s_result = M.serial(o, ids, owned)
    assert set(np.unique(s_outcome)) >= ({0, 1, 3, 4} if owned is None else {0, 1, 2, 3, 4})
    assert np.array_equal(outcome, s_outcome), np.nonzero(outcome != s_outcome)[0][:10]
    assert result == s_result and result["dropped"] > 0
    assert p.tobytes() == o.particles.tobytes()
    assert qi.tobytes() == o.queue_info.tobytes()
    assert q.tobytes() == o.queue.tobytes()
    o.close()
