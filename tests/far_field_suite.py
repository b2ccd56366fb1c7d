"""The field services on far contexts, what the suites of the three methods share (test_gpu_far_potential.py: flat and pyramid;
test_gpu_far_quad_potential.py: quadrupole; include/psamd.h: "energy", "the field at chosen points", "quadrupoles on the pyramid"):
phi and U against the numpy model (far_model.py; 1e-5 relative, the standing bar of every far phi) and the first phi against the
model's fp32 association, a confined cloud (the cutoff context's bytes), ACC probes against the force records and PHI probes on
kids against psamd_potential BIT FOR BIT, the same bytes however the call is made, the calls in a captured graph, the statuses.

METHODS has one row per method.  Every check below is written once and takes the method; tests_of(*methods) makes the rows' cases
of them into test functions, which a suite takes into its namespace -- under the names its nodes have had -- beside the tests only
its methods have.  The contexts, grids and clouds are far_harness.py's."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import far_model as F
import particlesystem_amd as ps
from far_harness import (DEV, INVALID_ARG, STATE, UNSUPPORTED, bits, body_cloud, box_cloud, by_fill, fill_lists, make, open_frame,
                         pos4_of, record, served)
from service_harness import captured
from util import assert_same_particles

MONO, PYR = ps.FLAG_FAR_MONOPOLE, ps.FLAG_FAR_PYRAMID
QUAD = PYR | ps.FLAG_FAR_QUADRUPOLE
FAST = ps.FLAG_FAST_MATH
PQ = ps.POTENTIAL_FAR | ps.POTENTIAL_QUADRUPOLE
ACC, PHI, PFAR, PQUAD = ps.PROBE_ACC, ps.PROBE_PHI, ps.PROBE_FAR, ps.PROBE_QUADRUPOLE
REL = 1e-5
EPS2 = 0.2
OF_FLAGS = {MONO: "flat", PYR: "pyramid", QUAD: "quadrupole"}          # (far_model.py's names)

# method (far_model.py's name): its row.
#   flags       of a context of the method
#   pot, mod    the bits of its own far form: psamd_potential's flags, psamd_probe's modifiers
#   beyond      the next bit the potential / the probe does not know on such a context
#   seed        a scene on G^3 cells is the cloud of seed + G ...
#   bodies      ... of {G: bodies}; 24 and 36 are far_harness.DEEP's grids of four and five levels (test_gpu_far_rough.py)
#   phi         the cases of phi_and_U_follow_the_model: {node id: (G, sign)}
#   confined    (G, bodies) of the confined cloud; G None: the default context's 16^3
#   probes      the cases of the probes' two checks: {node id: (G, FAST or 0)}
#   capture     whether the captured graph holds a probe call behind the potential's
#   strangers   the flags of the contexts that must take the method's bits for unknown ones
METHODS = {
    "flat": dict(
        flags=MONO, pot=ps.POTENTIAL_FAR, mod=PFAR, beyond=(0x2, 0x8), seed=40, bodies={8: 6000, 10: 8000, 16: 16384},
        phi={"%d-%s-flat" % c: c for c in [(8, 1.0), (8, -1.0), (10, 1.0), (16, 1.0), (16, -1.0)]}, confined=(None, 3000),
        probes={"flat-8": (8, 0), "flat-16": (16, 0)}, capture=False, strangers=(0, ps.FLAG_ALL_PAIRS)),
    "pyramid": dict(
        flags=PYR, pot=ps.POTENTIAL_FAR, mod=PFAR, beyond=(0x2, 0x8), seed=40, bodies={8: 6000, 10: 8000, 16: 16384, 24: 13824, 36: 16000},
        phi={"%d-%s-pyramid" % c: c for c in [(8, 1.0), (8, -1.0), (10, 1.0), (16, 1.0), (16, -1.0)]}, confined=(None, 3000),
        probes={"pyramid-10": (10, 0), "pyramid-16": (16, 0)}, capture=False, strangers=(0, ps.FLAG_ALL_PAIRS)),
    "quadrupole": dict(
        flags=QUAD, pot=PQ, mod=PFAR | PQUAD, beyond=(0x4, 0x10), seed=60,
        bodies={6: 3456, 8: 8192, 10: 16000, 16: 16384, 24: 13824, 36: 16000},
        phi={"%d-%s" % c: c for c in [(6, 1.0), (6, -1.0), (8, 1.0), (8, -1.0), (10, 1.0), (10, -1.0)]}, confined=(8, 320),
        probes={"%d-%s" % (G, "fast" if fast else "exact"): (G, fast) for G in (8, 10, 16) for fast in (0, FAST)}, capture=True,
        strangers=(0, ps.FLAG_ALL_PAIRS, MONO, PYR)),
}


@functools.lru_cache(maxsize=None)
def scene(G, flags, sign, seed, n):
    """one frame of a cloud with kids on a far context, everything the tests compare: the context's far phi (order of the fill)
    and its record, ACC probes on the adults (sorted order) and PHI probes on the kids, the force records (sorted order), the
    lists, the model's moments.  Computed once, never changed."""
    c = body_cloud(n, seed, G)
    g = make(G, flags, force_sign=sign)
    ids = g.fill_particles(**c)
    open_frame(g)
    how = served(g, True)
    res = g.download_potential(**how)
    lists, order = fill_lists(g, ids)
    assert len(order) == n and g.counters["cell_overflow_kills"] == 0
    kid = c["age"] < 1.5
    adults = order[~kid[order]]
    acc = g.probe(pos4_of(c["xyz"][adults]), phi=False, **how)
    kids = np.nonzero(kid)[0]
    phi_kids = g.probe(pos4_of(c["xyz"][kids]), acc=False, **how)
    g.calc_forces_pairs()
    f = g.download_force4(0, n)
    g.calc_forces_apply()
    g.close()
    w_eff = np.where(kid, np.float32(0.0), np.float32(sign) * c["w"]).astype(np.float32)
    return dict(c=c, ids=ids, res=res, phi=by_fill(ids, res["phi"]), lists=lists, order=order, f=f, kid=kid, w_eff=w_eff,
                cell=F.cells_of(c["xyz"], G), adults=adults, acc=acc, kids=kids, phi_kids=phi_kids,
                moments=F.level_moments(lists, c["xyz"], w_eff, G, OF_FLAGS[flags & ~FAST]))


def scene_of(method, G, sign=1.0, fast=0):
    """the method's own scene on G^3 cells"""
    row = METHODS[method]
    return scene(int(G), int(row["flags"] | fast), float(sign), int(row["seed"] + G), int(row["bodies"][G]))


# ---- 1. against the model -----------------------------------------------------------------------------------------------

def phi_and_U_follow_the_model(method, G, sign):
    """kids present (they are given the field at their own position), unequal masses; repulsion flips phi and U together.
    Measured on an MI355X on quadrupole contexts, max relative deviation of phi from the model / of U / of the first 400 phi from
    the model's fp32 association:
    6^3 1.5e-7 / 1.1e-8 / 1.1e-7;  8^3 3.8e-7 / 9.7e-9 / 1.9e-7;  10^3 1.8e-7 / 6.5e-9 / 1.4e-7  (either sign)"""
    s = scene_of(method, G, sign)
    n = len(s["ids"])
    xyz = s["c"]["xyz"]
    want = F.phi64(s["lists"], xyz, s["w_eff"], G, EPS2, xyz, s["cell"], np.arange(n), method, s["moments"])
    rel = np.abs(s["phi"].astype(np.float64) - want) / np.abs(want)
    U = F.energy(s["w_eff"], want)
    near = F.phi64(s["lists"], xyz, s["w_eff"], G, EPS2, xyz[:200], s["cell"][:200], np.arange(200), method, far=False)
    faith = F.phi32(s["lists"], xyz, s["w_eff"], G, EPS2, xyz[:400], s["cell"][:400], np.arange(400), method, s["moments"])
    rel32 = np.abs(s["phi"][:400].astype(np.float64) - faith) / np.abs(faith)
    print("%s far phi, %d bodies on %d^3 cells, sign %+.0f: max relative deviation from the model %.3g, U %.3g; from the "
          "model's fp32 association %.3g; the stencil alone is %.3g of phi (median)"
          % (method, n, G, sign, rel.max(), abs(s["res"]["potential"] - U) / abs(U), rel32.max(), np.median(near / want[:200])))
    assert s["res"]["listed"] == n and s["res"]["nonfinite"] == 0 and s["kid"].sum() > 100
    assert (np.sign(want) == -sign).all() and np.median(near / want[:200]) < 0.5      # (the far part is no small correction)
    assert rel.max() < REL
    assert abs(s["res"]["potential"] - U) < REL * abs(U)
    assert rel32.max() < F.ALLOW
    assert s["res"]["phi_min"] == float(s["phi"].min()) and s["res"]["phi_max"] == float(s["phi"].max())


# ---- 2. no far body: the cutoff context's bytes ----------------------------------------------------------------------------------

def confined_cloud_is_the_cutoff_context_byte_for_byte(*methods):
    """a cloud inside the 2x2x2 block of cells around the origin -- of the default 16^3 grid, or of 8^3 (one corner segment of the
    small context: 8 lists of 66, so 320 bodies, 40 a cell) --: no far body at any level, whatever the planes hold"""
    G, n = METHODS[methods[0]]["confined"]
    assert all(METHODS[m]["confined"] == (G, n) for m in methods)
    rng = np.random.default_rng(7)
    xyz = rng.uniform(-4.99, 4.99, (n, 3)).astype(np.float32)
    age = rng.uniform(0.5, 7.5, n).astype(np.float32)
    got = []
    for flags in [0] + [METHODS[m]["flags"] for m in methods]:
        g = make(G, flags) if G else ps.ParticleSystem(ps.default_config(flags=flags))
        g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
        open_frame(g)
        how = served(g, flags != 0)
        got.append((g.potential(phi=True, **how), g.download_potential(**how), g.probe(pos4_of(xyz), **how)["out4"]))
        g.calc_forces()
        if G:
            assert g.counters["cell_overflow_kills"] == 0                 # (the small context's lists hold the cloud)
        g.close()
    base = got[0][0]
    assert base["listed"] == n and base["potential"] < 0 and (age < 1.5).sum() > 20
    for pot, down, out4 in got:
        for r in (pot, down):
            assert np.array_equal(bits(r["phi"]), bits(base["phi"])) and record(r) == record(base)
        assert np.array_equal(bits(out4), bits(got[0][2]))


# ---- 3. the probes repeat the force records and psamd_potential, bit for bit -------------------------------------------------------

def acc_probes_on_served_adults_are_their_force_records_bit_for_bit(method, G, fast=0):
    """ACC probes of the method's far form on every served adult against download_force4's records.  8^3 flat: 8 blocks over 16
    parts; 16^3: 64 blocks, 4 a part, and as a pyramid level 0 of 64 blocks and level 1 of 8.  At 16^3 there are 4 bodies a cell:
    a wave of 64 probes sits in some 16 cells under several parents"""
    s = scene_of(method, G, fast=fast)
    adults = s["adults"]
    f = s["f"][~s["kid"][s["order"]]]
    assert (f[:, 3].view(np.int32) == 0).all() and np.abs(f[:, :3]).max() > 0      # (every adult was served: no collision)
    got = s["acc"]["out4"].cpu().numpy()
    assert s["acc"]["served"] == len(adults) > 0 and s["acc"]["nonfinite"] == 0 and not got[:, 3].any()
    if G == 16:
        first = s["cell"][adults[:64]]                                    # (sorted order: cell-major, as the probes are served)
        i1, i2, i3 = (first // G % G) >> 1, (first % G) >> 1, (first // (G * G)) >> 1
        assert len(np.unique(first)) >= 8 and len(np.unique((i3 * 8 + i1) * 8 + i2)) >= 2      # one wave: many cells, more than one parent
    bad = np.nonzero((bits(got[:, :3]) != bits(f[:, :3])).any(1))[0]
    assert len(bad) == 0, "%d of %d probes differ from the force record, first %d: probe %r record %r" % (len(bad), len(f), bad[0], got[bad[0]], f[bad[0]])


def phi_probes_on_kids_are_the_kids_phi_bit_for_bit(method, G, fast=0):
    """PHI probes at the listed kids' true positions against their phi from psamd_potential"""
    s = scene_of(method, G, fast=fast)
    on = s["phi_kids"]["out4"].cpu().numpy()
    assert s["phi_kids"]["served"] == len(s["kids"]) > 100 and not on[:, :3].any()
    assert np.array_equal(bits(on[:, 3]), bits(s["phi"][s["kids"]]))


def probes_repeat_the_force_records_and_the_kids_phi_bit_for_bit(method, G, fast):
    acc_probes_on_served_adults_are_their_force_records_bit_for_bit(method, G, fast)
    phi_probes_on_kids_are_the_kids_phi_bit_for_bit(method, G, fast)


# ---- 4. the same bytes however it is called ---------------------------------------------------------------------------------------

def the_same_bytes_before_and_after_the_pair_stage_and_nothing_else_moves(method):
    G = 8
    flags = METHODS[method]["flags"]
    s = scene_of(method, G)
    g = make(G, flags)
    b = make(G, flags)                                                    # never makes a far call
    for x in (g, b):
        x.fill_particles(**s["c"])
        open_frame(x)
    how = served(g, True)
    pts = pos4_of(s["c"]["xyz"][:1000])
    first = g.potential(phi=True, **how)
    again = g.potential(phi=True, **how)
    p1 = g.probe(pts, **how)["out4"]
    g.calc_forces_pairs(); b.calc_forces_pairs()                          # (the window stays open behind the pair stage)
    after = g.download_potential(**how)
    p2 = g.probe(pts, **how)["out4"]
    n = len(s["ids"])
    fa, fb = g.download_force4(0, n), b.download_force4(0, n)
    mom = [x.download_level_moments(0) if flags & PYR else x.download_cell_moments() for x in (g, b)]
    g.calc_forces_apply(); b.calc_forces_apply()
    g.step(1); b.step(1)
    for r in (again, after):
        assert np.array_equal(bits(r["phi"]), bits(first["phi"])) and record(r) == record(first)
    assert np.array_equal(bits(first["phi"]), bits(s["res"]["phi"])) and np.array_equal(bits(p1), bits(p2))
    assert fa.tobytes() == fb.tobytes() == s["f"].tobytes() and mom[0].tobytes() == mom[1].tobytes()
    assert_same_particles(g.download_particles(), b.download_particles(), "a step after far potential calls")
    assert g.counters == b.counters
    g.close(); b.close()


def the_calls_are_captured_into_a_graph_and_replay_on_a_later_frame(method):
    """psamd_potential -- and, where the row says so, psamd_probe behind it -- of the method's far form"""
    row = METHODS[method]
    G, m = 8, 1024
    g = make(G, row["flags"])
    c = body_cloud(6000, 48, G)
    g.fill_particles(**c, vxyz=box_cloud(6000, 49, 2.0))
    g.step(1)
    open_frame(g)
    how = served(g, True)
    cap = g.owned_slots()
    if row["capture"]:
        pts = pos4_of(box_cloud(m, 50, G))
        g.probe(pts, **how)                                               # (the probes' scratch has grown: nothing to allocate under the capture)
        out4 = torch.zeros((m, 4), dtype=torch.float32, device=DEV)
        prec = torch.zeros(C.sizeof(ps.ProbeResult), dtype=torch.uint8, device=DEV)
        pspec = ps.ProbeSpec(fields=ACC | PHI | row["mod"], max_count=m, pos4=pts.data_ptr(), out4=out4.data_ptr(), result_dev=prec.data_ptr())
    phi = torch.zeros(cap, dtype=torch.float32, device=DEV)
    rec = torch.zeros(C.sizeof(ps.PotentialResult), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    spec = ps.Potential(flags=row["pot"], phi=phi.data_ptr(), capacity=cap, result_dev=rec.data_ptr())
    with captured(g) as cap:
        rc = g.lib.psamd_potential(g.h, C.byref(spec))
        rp = g.lib.psamd_probe(g.h, C.byref(pspec)) if row["capture"] else 0
    assert rc == 0 and rp == 0
    g.calc_forces()
    g.step(2)
    open_frame(g)                                                         # another frame: the graph holds nothing of the one it was captured in
    cap.launch()
    replayed = ps.PotentialResult.from_buffer_copy(rec.cpu().numpy().tobytes()).to_dict()
    eager = g.potential(phi=True, **how)
    assert replayed == record(eager) == g.potential_result()
    assert replayed["listed"] == len(eager["phi"]) > 0
    assert np.array_equal(bits(phi[:len(eager["phi"])]), bits(eager["phi"]))
    if row["capture"]:
        probed = ps.ProbeResult.from_buffer_copy(prec.cpu().numpy().tobytes()).to_dict()
        again = g.probe(pts, **how)
        assert probed == {k: again[k] for k in probed} and probed["served"] == m
        assert np.array_equal(bits(out4), bits(again["out4"])) and np.abs(out4.cpu().numpy()).min() > 0
    cap.close()
    g.calc_forces()
    g.synchronize()
    g.close()


# ---- 5. the statuses ----------------------------------------------------------------------------------------------------------

def pot_status(g, flags, **kw):
    return g.lib.psamd_potential(g.h, C.byref(ps.Potential(flags=flags, **kw)))


def host_status(g, flags, capacity=0, result=None):
    return g.lib.psamd_download_potential_flags(g.h, flags, None, capacity, result)


def probe_status(g, fields, max_count=0):
    return g.lib.psamd_probe(g.h, C.byref(ps.ProbeSpec(fields=fields, max_count=max_count)))


def bits_the_context_does_not_know(flags):
    """a context that serves no far form, or FAR alone: every set of the far bits with one it does not know is INVALID_ARG, and
    the host form with the flags it knows is the old forms' call"""
    g = make(8, flags)
    g.fill_particles(**body_cloud(2000, 71, 8))
    open_frame(g)
    far = flags in (MONO, PYR)
    for f in (ps.POTENTIAL_FAR, ps.POTENTIAL_QUADRUPOLE, PQ):
        if not far or f != ps.POTENTIAL_FAR:
            assert pot_status(g, f) == INVALID_ARG and host_status(g, f) == INVALID_ARG, f
    for f in (PFAR, PQUAD, PFAR | PQUAD):
        if not far or f != PFAR:
            assert probe_status(g, ACC | f) == INVALID_ARG and probe_status(g, ACC | PHI | f) == INVALID_ARG, f
    r = ps.PotentialResult()
    if far:
        assert host_status(g, 0) == UNSUPPORTED
        want = g.download_potential(phi=False, far=True)
        assert host_status(g, ps.POTENTIAL_FAR, 0, C.byref(r)) == 0 and r.to_dict() == want
    else:
        assert g.lib.psamd_download_potential_far(g.h, None, 0, None) == UNSUPPORTED      # (as before)
        want = g.download_potential(phi=False)                            # the context stayed usable
        assert host_status(g, 0, 0, C.byref(r)) == 0 and r.to_dict() == want and want["listed"] == 2000
    g.calc_forces()
    g.close()


def the_methods_own_statuses(method):
    row = METHODS[method]
    pot, mod = row["pot"], row["mod"]
    old_far = lambda capacity=0: g.lib.psamd_download_potential_far(g.h, None, capacity, None)      # (the host form of FAR alone)
    c = body_cloud(2000, 71, 8)
    g = make(8, row["flags"])
    g.fill_particles(**c)
    assert pot_status(g, pot) == STATE and host_status(g, pot) == STATE      # outside the window
    assert probe_status(g, ACC | mod) == STATE and probe_status(g, PHI | mod) == STATE
    assert pot != ps.POTENTIAL_FAR or old_far() == STATE
    open_frame(g)
    how = served(g, True)
    # QUADRUPOLE without FAR -- a modifier without what it modifies, or a bit the context does not know --, modifiers alone, a bit beyond
    assert pot_status(g, ps.POTENTIAL_QUADRUPOLE) == INVALID_ARG and host_status(g, ps.POTENTIAL_QUADRUPOLE) == INVALID_ARG
    assert probe_status(g, ACC | PQUAD) == INVALID_ARG
    assert probe_status(g, mod) == INVALID_ARG
    assert pot_status(g, pot | row["beyond"][0]) == INVALID_ARG
    assert probe_status(g, ACC | mod | row["beyond"][1]) == INVALID_ARG
    # fewer bits than the context's own form: not this context's field
    for f in {0, pot & ps.POTENTIAL_FAR} - {pot}:
        assert pot_status(g, f) == UNSUPPORTED and host_status(g, f) == UNSUPPORTED, f
    assert g.lib.psamd_download_potential(g.h, None, 0, None) == UNSUPPORTED
    assert pot == ps.POTENTIAL_FAR or old_far() == UNSUPPORTED
    for less in {0, mod & PFAR} - {mod}:
        for f in (ACC, PHI, ACC | PHI):
            assert probe_status(g, f | less) == UNSUPPORTED, (f, less)
    # the own form: served, with psamd_potential's and psamd_probe's arguments
    assert pot_status(g, pot, capacity=-1) == INVALID_ARG
    assert pot_status(g, pot, reserved=1) == INVALID_ARG
    assert host_status(g, pot, 5) == INVALID_ARG and host_status(g, pot, -1) == INVALID_ARG
    assert pot != ps.POTENTIAL_FAR or old_far(5) == INVALID_ARG
    assert probe_status(g, ACC | mod, 4) == INVALID_ARG                   # no arrays
    assert pot_status(g, pot) == 0
    dev = torch.full((5,), 7, dtype=torch.int64, device=DEV)
    spec = ps.ProbeSpec(fields=ACC | PHI | mod, max_count=0)
    spec.result_dev = dev.data_ptr()
    assert g.lib.psamd_probe(g.h, C.byref(spec)) == 0                     # max_count == 0: a zero result
    g.synchronize()
    assert not dev.cpu().numpy().any() and not any(g.probe_result().values())
    r = ps.PotentialResult()
    assert host_status(g, pot, 0, C.byref(r)) == 0
    down = g.download_potential(**how)
    assert r.to_dict() == record(down) == g.potential_result() and down["listed"] == len(down["phi"]) == 2000
    e = g.energy(**how)
    assert e["potential"] == down["potential"] == g.download_potential(phi=False, **how)["potential"] < 0
    assert e["total"] == e["kinetic"] + e["potential"]
    assert g.probe(pos4_of(c["xyz"][:64]), **how)["served"] == 64
    g.calc_forces_pairs(); g.calc_forces_apply()
    assert pot_status(g, pot) == STATE                                    # the frame has ended
    g.step(1); g.synchronize()                                            # the context steps on
    assert g.live_count() >= 1950
    g.close()


def the_status_table_cell_by_cell(*methods):
    for flags in sorted({f for m in methods for f in METHODS[m]["strangers"]}):
        bits_the_context_does_not_know(flags)
    for method in methods:
        the_methods_own_statuses(method)


# ---- the cases of the rows as tests ---------------------------------------------------------------------------------------------

def tests_of(*methods):
    """{the name of a check: its test function over the cases of the rows of `methods`}, for the namespace of their suite.  A check
    with one case per method is parametrised by the method's name where the suite has several; the checks that open a cutoff
    context or the strangers take all the suite's methods in one test"""
    def over(check, cases):
        """cases: {node id: arguments}; one case without an id: a plain test"""
        if list(cases) == [None]:
            def test():
                check(*cases[None])
        else:
            @pytest.mark.parametrize("case", [pytest.param(args, id=i) for i, args in cases.items()])
            def test(case):
                check(*case)
        test.__doc__ = check.__doc__
        return test

    each = {m if len(methods) > 1 else None: (m,) for m in methods}
    return dict(
        phi_and_U_follow_the_model=over(phi_and_U_follow_the_model, {i: (m,) + c for m in methods for i, c in METHODS[m]["phi"].items()}),
        confined_cloud_is_the_cutoff_context_byte_for_byte=over(confined_cloud_is_the_cutoff_context_byte_for_byte, {None: methods}),
        probes_repeat_the_force_records_and_the_kids_phi_bit_for_bit=over(
            probes_repeat_the_force_records_and_the_kids_phi_bit_for_bit, {i: (m,) + c for m in methods for i, c in METHODS[m]["probes"].items()}),
        the_same_bytes_before_and_after_the_pair_stage_and_nothing_else_moves=over(the_same_bytes_before_and_after_the_pair_stage_and_nothing_else_moves, each),
        the_calls_are_captured_into_a_graph_and_replay_on_a_later_frame=over(the_calls_are_captured_into_a_graph_and_replay_on_a_later_frame, each),
        the_status_table_cell_by_cell=over(the_status_table_cell_by_cell, {None: methods}))
