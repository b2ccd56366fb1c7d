"""PSAMD_POTENTIAL_FAR | PSAMD_POTENTIAL_QUADRUPOLE and PSAMD_PROBE_FAR | PSAMD_PROBE_QUADRUPOLE on the device (include/psamd.h,
"energy", "the field at chosen points" and "quadrupoles on the pyramid"): phi and U against the numpy model
(far_quad_field_model.py; 1e-5 relative, the standing bar of every far phi), the quadrupole part alone, the probes against the
force records and against psamd_potential BIT FOR BIT, the two exact limits (every C a zero: the pyramid context's bytes; a
confined cloud: the cutoff context's), the same bytes however the call is made, and the statuses.

Contexts hold max_particles_num=16384 (far_harness.py's GRID): 4^3 (one level), 6^3 (6, 3), 8^3 (8, 4), 10^3 (10, 5, 3: ragged) and
16^3 (16, 8, 4: levels of several blocks).

What was measured on an MI355X stands in the tests' docstrings."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import far_model as F
import far_quad_field_model as Q
import particlesystem_amd as ps
from far_harness import GRID, INVALID_ARG, STATE, UNSUPPORTED, box_cloud, fill_lists, hip_runtime, low_corner, open_frame

pytestmark = pytest.mark.gpu

PYR, MONO = ps.FLAG_FAR_PYRAMID, ps.FLAG_FAR_MONOPOLE
QUAD = PYR | ps.FLAG_FAR_QUADRUPOLE
FAST = ps.FLAG_FAST_MATH
PQ = ps.POTENTIAL_FAR | ps.POTENTIAL_QUADRUPOLE
REL = 1e-5
EPS2 = 0.2
DEV = torch.device("cuda", 0)
BODIES = {6: 3456, 8: 8192, 10: 16000, 16: 16384}


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make(G, flags, **over):
    g = ps.ParticleSystem(ps.default_config(flags=flags, collision_radius=1e-6, **GRID[G], **over))
    assert g.sizes.grid_dim == G
    return g


def body_cloud(n, seed, G):
    """kids among the adults (they exert nothing and get the field at their own place), unequal masses"""
    rng = np.random.default_rng(seed)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    age[::17] = 0.5
    return dict(xyz=box_cloud(n, seed, G), age=age, w=rng.uniform(20.0, 100.0, n).astype(np.float32), fert_age=np.float32(1e6))


def by_fill(ids, phi):
    """phi pairs with the live particles in ascending slot id: back to the order of the fill"""
    out = np.empty(len(ids), np.float32)
    out[np.argsort(ids)] = np.asarray(phi.cpu().numpy() if isinstance(phi, torch.Tensor) else phi)
    return out


def pos4_of(xyz):
    p = np.zeros((len(xyz), 4), np.float32)
    p[:, :3] = xyz
    return torch.from_numpy(p).to(DEV)


def record(res):
    return {k: res[k] for k in res if k != "phi"}


def served(g, far):
    """the potential and the probe keywords of a context's own far form"""
    return dict(far=far, quadrupole=bool(g.cfg.flags & ps.FLAG_FAR_QUADRUPOLE))


def scene(G, flags=QUAD, sign=1.0, seed=None, n=None):
    return _scene(int(G), int(flags), float(sign), int(60 + G if seed is None else seed), int(BODIES[G] if n is None else n))


@functools.lru_cache(maxsize=None)
def _scene(G, flags, sign, seed, n):
    """one frame of a cloud with kids on a far context, everything the tests below compare: the context's far phi (order of the
    fill) and its record, ACC probes on the adults (sorted order) and PHI probes on the kids, the force records (sorted order),
    the lists.  Computed once, never changed."""
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
                cell=F.cells_of(c["xyz"], G), adults=adults, acc=acc, kids=kids, phi_kids=phi_kids)


# ---- 1. against the model -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,sign", [(6, 1.0), (6, -1.0), (8, 1.0), (8, -1.0), (10, 1.0), (10, -1.0)])
def test_phi_and_U_follow_the_model(G, sign):
    """kids present, unequal masses; repulsion flips phi and U together.  Measured on an MI355X, max relative deviation of phi
    from the model / of U / of the first 400 phi from the model's fp32 association:
    6^3 1.5e-7 / 1.1e-8 / 1.1e-7;  8^3 3.8e-7 / 9.7e-9 / 1.9e-7;  10^3 1.8e-7 / 6.5e-9 / 1.4e-7  (either sign)"""
    s = scene(G, QUAD, sign)
    n = len(s["ids"])
    xyz = s["c"]["xyz"]
    moments = F.level_moments(s["lists"], xyz, s["w_eff"], G, "quadrupole")
    want = Q.phi64(s["lists"], xyz, s["w_eff"], G, EPS2, xyz, s["cell"], np.arange(n), moments)
    rel = np.abs(s["phi"].astype(np.float64) - want) / np.abs(want)
    U = F.energy(s["w_eff"], want)
    faith = Q.phi32(s["lists"], xyz, s["w_eff"], G, EPS2, xyz[:400], s["cell"][:400], np.arange(400), moments)
    rel32 = np.abs(s["phi"][:400].astype(np.float64) - faith) / np.abs(faith)
    print("quadrupole far phi, %d bodies on %d^3 cells, sign %+.0f: max relative deviation from the model %.3g, U %.3g; from the "
          "model's fp32 association %.3g" % (n, G, sign, rel.max(), abs(s["res"]["potential"] - U) / abs(U), rel32.max()))
    assert s["res"]["listed"] == n and s["res"]["nonfinite"] == 0 and s["kid"].sum() > 100
    assert (np.sign(want) == -sign).all()
    assert rel.max() < REL
    assert abs(s["res"]["potential"] - U) < REL * abs(U)
    assert s["res"]["phi_min"] == float(s["phi"].min()) and s["res"]["phi_max"] == float(s["phi"].max())


# ---- 2. the quadrupole part alone -----------------------------------------------------------------------------------------------

def test_the_quadrupole_part_alone():
    """8^3 cells, 16384 bodies (seed 52: chosen with the model on the CPU, where 60 % of the particles have a quadrupole part of at
    least 1e-4 of |phi|; median 1.25e-4).  phi of a quadrupole context under FAR | QUADRUPOLE minus phi of a pyramid context under
    FAR on the same cloud is the quadrupole chains' sum up to the fp32 rounding of the two records: about 1.2e-7 |phi|, which is
    1.2e-3 of a part of 1e-4 |phi|.  The bar of 1e-2 of the part leaves some 8 times that; a wrong coefficient or a swapped plane
    moves the part by tens of percent.  Measured on an MI355X: 59.7 % of the
    particles qualify; over them the difference is off by at most 9.3e-4 of the part (median 1.3e-4)"""
    G, n, seed = 8, 16384, 52
    a, b = scene(G, QUAD, seed=seed, n=n), scene(G, PYR, seed=seed, n=n)
    assert np.array_equal(a["order"], b["order"])
    xyz = a["c"]["xyz"]
    moments = F.level_moments(a["lists"], xyz, a["w_eff"], G, "quadrupole")
    part = -Q.quad_sum64(a["lists"], xyz, a["w_eff"], G, EPS2, xyz, a["cell"], moments)      # (phi = -sum)
    got = a["phi"].astype(np.float64) - b["phi"].astype(np.float64)
    big = np.abs(part) >= 1e-4 * np.abs(a["phi"])
    rel = np.abs(got[big] - part[big]) / np.abs(part[big])
    print("the quadrupole part of phi alone, %d bodies on %d^3 cells: %.3f of the particles have a part of at least 1e-4 |phi|; over "
          "them, max deviation from the model's part %.3g of the part (median %.3g)" % (n, G, big.mean(), rel.max(), np.median(rel)))
    assert big.mean() >= 0.25
    assert rel.max() < 1e-2


# ---- 3. the probes repeat the force records and psamd_potential, bit for bit -------------------------------------------------------

@pytest.mark.parametrize("fast", [0, FAST], ids=["exact", "fast"])
@pytest.mark.parametrize("G", [8, 10, 16])
def test_probes_repeat_the_force_records_and_the_kids_phi_bit_for_bit(G, fast):
    """ACC | FAR | QUADRUPOLE probes on every served adult against download_force4's records, PHI probes at the listed kids' true
    positions against their phi from psamd_potential.  16^3: three levels, level 0 of 64 blocks, 4 bodies a cell -- a wave of 64
    probes sits in some 16 cells under several parents"""
    s = scene(G, QUAD | fast)
    f = s["f"][~s["kid"][s["order"]]]
    assert (f[:, 3].view(np.int32) == 0).all() and np.abs(f[:, :3]).max() > 0      # (every adult was served: no collision)
    got = s["acc"]["out4"].cpu().numpy()
    assert s["acc"]["served"] == len(s["adults"]) > 0 and s["acc"]["nonfinite"] == 0 and not got[:, 3].any()
    bad = np.nonzero((bits(got[:, :3]) != bits(f[:, :3])).any(1))[0]
    assert len(bad) == 0, "%d of %d probes differ from the force record, first %d: probe %r record %r" % (len(bad), len(f), bad[0], got[bad[0]], f[bad[0]])
    on = s["phi_kids"]["out4"].cpu().numpy()
    assert s["phi_kids"]["served"] == len(s["kids"]) > 100 and not on[:, :3].any()
    assert np.array_equal(bits(on[:, 3]), bits(s["phi"][s["kids"]]))


# ---- 4. every C an exact zero: the pyramid context's bytes --------------------------------------------------------------------------

def test_one_adult_a_cell_is_the_pyramid_context_byte_for_byte():
    """4^3 cells with one adult each and 300 kids anywhere: every C is an exact zero and every quadrupole chain +0"""
    G = 4
    rng = np.random.default_rng(5)
    adults = np.array([low_corner(i1, i2, i3, G) for i3 in range(G) for i1 in range(G) for i2 in range(G)]) + rng.uniform(0.1, 4.9, (G ** 3, 3))
    xyz = np.concatenate([adults, rng.uniform(-9.9, 9.9, (300, 3))]).astype(np.float32)
    age = np.concatenate([np.full(G ** 3, 3.0), np.full(300, 0.5)]).astype(np.float32)
    w = rng.uniform(20.0, 100.0, len(xyz)).astype(np.float32)
    grid = pos4_of(rng.uniform(-9.9, 9.9, (500, 3)).astype(np.float32))
    got = []
    for flags in (QUAD, PYR):
        g = make(G, flags)
        g.fill_particles(xyz, age=age, w=w, fert_age=np.float32(1e6))
        open_frame(g)
        how = served(g, True)
        got.append((g.potential(phi=True, **how), g.probe(pos4_of(xyz), **how), g.probe(grid, **how)))
        g.calc_forces_pairs()
        if flags == QUAD:
            cen = g.download_level_quadrupoles(0)
            assert cen.shape == (G ** 3, 6) and not cen.view(np.uint32).any()      # (+0, every word)
            assert (g.download_level_moments(0)[:, 3] != 0).all()
        g.calc_forces_apply()
        g.close()
    (pa, oa, ga), (pb, ob, gb) = got
    assert pa["listed"] == len(xyz) and pa["potential"] < 0 and record(pa) == record(pb)
    assert np.array_equal(bits(pa["phi"]), bits(pb["phi"]))
    for x, y in ((oa, ob), (ga, gb)):
        assert x["served"] == y["served"] == len(x["out4"]) and np.array_equal(bits(x["out4"]), bits(y["out4"]))
    assert np.abs(oa["out4"].cpu().numpy()).min() > 0


# ---- 5. no far body: the cutoff context's bytes ----------------------------------------------------------------------------------

def test_a_confined_cloud_is_the_cutoff_context_byte_for_byte():
    """a cloud inside the 2x2x2 block of cells 3..4 of 8^3 (one corner segment of the small context: 8 lists of 66, so 320 bodies,
    40 a cell): no far body at any level, whatever the planes hold"""
    G, n = 8, 320
    rng = np.random.default_rng(7)
    xyz = rng.uniform(-4.99, 4.99, (n, 3)).astype(np.float32)
    age = rng.uniform(0.5, 7.5, n).astype(np.float32)
    got = []
    for flags in (0, QUAD):
        g = make(G, flags)
        g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
        open_frame(g)
        how = served(g, flags != 0)
        got.append((g.potential(phi=True, **how), g.download_potential(**how), g.probe(pos4_of(xyz), **how)["out4"]))
        g.calc_forces()
        assert g.counters["cell_overflow_kills"] == 0
        g.close()
    assert got[0][0]["listed"] == n and got[0][0]["potential"] < 0 and (age < 1.5).sum() > 20
    for r in (got[0][1], got[1][0], got[1][1]):
        assert np.array_equal(bits(r["phi"]), bits(got[0][0]["phi"])) and record(r) == record(got[0][0])
    assert np.array_equal(bits(got[0][2]), bits(got[1][2]))


# ---- 6. the same bytes however it is called ---------------------------------------------------------------------------------------

def test_two_calls_shuffled_probes_and_a_larger_max_count_give_the_same_bytes():
    G = 8
    s = scene(G)
    g = make(G, QUAD)
    g.fill_particles(**s["c"])
    open_frame(g)
    first = g.potential(phi=True, far=True, quadrupole=True)
    again = g.download_potential(far=True, quadrupole=True)
    m = 1500
    xyz = s["c"]["xyz"][:m]
    whole = g.probe(pos4_of(xyz), far=True, quadrupole=True)["out4"].cpu().numpy()
    g.calc_forces_pairs()                                                 # (the window stays open behind the pair stage)
    perm = np.random.default_rng(8).permutation(m)
    pad = np.concatenate([xyz[perm], np.full((700, 3), 1.0, np.float32)])
    count = torch.tensor([m], dtype=torch.int64, device=DEV)
    mixed = g.probe(pos4_of(pad), count=count, far=True, quadrupole=True)
    only_a = g.probe(pos4_of(xyz), phi=False, far=True, quadrupole=True)["out4"].cpu().numpy()
    only_p = g.probe(pos4_of(xyz), acc=False, far=True, quadrupole=True)["out4"].cpu().numpy()
    after = g.potential(phi=True, far=True, quadrupole=True)
    g.calc_forces_apply()
    g.close()
    for r in (again, after, s["res"]):
        assert np.array_equal(bits(r["phi"]), bits(first["phi"])) and record(r) == record(first)
    out = mixed["out4"].cpu().numpy()
    assert mixed["done"] == mixed["served"] == m and not out[m:].any()
    assert np.array_equal(bits(out[:m]), bits(whole[perm]))
    # where both are asked for, a body's front is formed once, in the acceleration's walk: the words of the walks of their own
    assert np.array_equal(bits(whole[:, :3]), bits(only_a[:, :3])) and np.array_equal(bits(whole[:, 3]), bits(only_p[:, 3]))
    assert np.abs(whole).min() > 0


def test_the_calls_are_captured_into_a_graph_and_replay_on_a_later_frame():
    G, m = 8, 1024
    g = make(G, QUAD)
    c = body_cloud(6000, 48, G)
    g.fill_particles(**c, vxyz=box_cloud(6000, 49, 2.0))
    g.step(1)
    open_frame(g)
    cap = g.owned_slots()
    pts = pos4_of(box_cloud(m, 50, G))
    g.probe(pts, far=True, quadrupole=True)                               # (the probes' scratch has grown: nothing to allocate under the capture)
    phi = torch.zeros(cap, dtype=torch.float32, device=DEV)
    rec = torch.zeros(C.sizeof(ps.PotentialResult), dtype=torch.uint8, device=DEV)
    out4 = torch.zeros((m, 4), dtype=torch.float32, device=DEV)
    prec = torch.zeros(C.sizeof(ps.ProbeResult), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    spec = ps.Potential(flags=PQ, phi=phi.data_ptr(), capacity=cap, result_dev=rec.data_ptr())
    pspec = ps.ProbeSpec(fields=ps.PROBE_ACC | ps.PROBE_PHI | ps.PROBE_FAR | ps.PROBE_QUADRUPOLE, max_count=m, pos4=pts.data_ptr(),
                         out4=out4.data_ptr(), result_dev=prec.data_ptr())
    hip = hip_runtime()
    stream = C.c_void_p(g.stream())
    graph, exe = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 2) == 0                      # hipStreamCaptureModeRelaxed
    rc = g.lib.psamd_potential(g.h, C.byref(spec))
    rp = g.lib.psamd_probe(g.h, C.byref(pspec))
    assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and rc == 0 and rp == 0
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
    g.calc_forces()
    g.step(2)
    open_frame(g)                                                         # another frame: the graph holds nothing of the one it was captured in
    assert hip.hipGraphLaunch(exe, stream) == 0
    assert hip.hipStreamSynchronize(stream) == 0
    replayed = ps.PotentialResult.from_buffer_copy(rec.cpu().numpy().tobytes()).to_dict()
    probed = ps.ProbeResult.from_buffer_copy(prec.cpu().numpy().tobytes()).to_dict()
    eager = g.potential(phi=True, far=True, quadrupole=True)
    assert replayed == record(eager) == g.potential_result()
    assert replayed["listed"] == len(eager["phi"]) > 0
    assert np.array_equal(bits(phi[:len(eager["phi"])]), bits(eager["phi"]))
    again = g.probe(pts, far=True, quadrupole=True)
    assert probed == {k: again[k] for k in probed} and probed["served"] == m
    assert np.array_equal(bits(out4), bits(again["out4"])) and np.abs(out4.cpu().numpy()).min() > 0
    assert hip.hipGraphExecDestroy(exe) == 0 and hip.hipGraphDestroy(graph) == 0
    g.calc_forces()
    g.synchronize()
    g.close()


# ---- 7. the statuses ----------------------------------------------------------------------------------------------------------

def test_the_status_table_cell_by_cell():
    c = body_cloud(2000, 71, 8)
    pot = lambda flags, **kw: ps.Potential(flags=flags, **kw)
    probe = lambda fields, m=0: ps.ProbeSpec(fields=fields, max_count=m)
    A, P, FAR, PQUAD = ps.PROBE_ACC, ps.PROBE_PHI, ps.PROBE_FAR, ps.PROBE_QUADRUPOLE
    for flags in (0, ps.FLAG_ALL_PAIRS, MONO, PYR):                       # no quadrupole context: either new bit is an unknown bit
        g = make(8, flags)
        g.fill_particles(**c)
        open_frame(g)
        far = ps.POTENTIAL_FAR if flags in (MONO, PYR) else 0             # (beside a bit the context knows, too)
        for f in {ps.POTENTIAL_QUADRUPOLE, ps.POTENTIAL_QUADRUPOLE | far}:
            assert g.lib.psamd_potential(g.h, C.byref(pot(f))) == INVALID_ARG
            assert g.lib.psamd_download_potential_flags(g.h, f, None, 0, None) == INVALID_ARG
        pfar = FAR if flags in (MONO, PYR) else 0
        for f in {A | PQUAD, A | P | PQUAD | pfar}:
            assert g.lib.psamd_probe(g.h, C.byref(probe(f))) == INVALID_ARG
        # the host form with flags the context knows is the old forms' call
        if far:
            assert g.lib.psamd_download_potential_flags(g.h, 0, None, 0, None) == UNSUPPORTED
            want = g.download_potential(phi=False, far=True)
            r = ps.PotentialResult()
            assert g.lib.psamd_download_potential_flags(g.h, far, None, 0, C.byref(r)) == 0 and r.to_dict() == want
        else:
            assert g.lib.psamd_download_potential_flags(g.h, ps.POTENTIAL_FAR, None, 0, None) == INVALID_ARG      # (as psamd_potential)
            assert g.lib.psamd_download_potential_far(g.h, None, 0, None) == UNSUPPORTED                           # (as before)
            r = ps.PotentialResult()
            assert g.lib.psamd_download_potential_flags(g.h, 0, None, 0, C.byref(r)) == 0 and r.to_dict() == g.download_potential(phi=False)
        g.calc_forces()
        g.close()
    g = make(8, QUAD)
    g.fill_particles(**c)
    assert g.lib.psamd_potential(g.h, C.byref(pot(PQ))) == STATE          # outside the window
    assert g.lib.psamd_download_potential_flags(g.h, PQ, None, 0, None) == STATE
    assert g.lib.psamd_probe(g.h, C.byref(probe(A | FAR | PQUAD))) == STATE
    open_frame(g)
    # a modifier without what it modifies
    assert g.lib.psamd_potential(g.h, C.byref(pot(ps.POTENTIAL_QUADRUPOLE))) == INVALID_ARG
    assert g.lib.psamd_download_potential_flags(g.h, ps.POTENTIAL_QUADRUPOLE, None, 0, None) == INVALID_ARG
    assert g.lib.psamd_probe(g.h, C.byref(probe(A | PQUAD))) == INVALID_ARG
    assert g.lib.psamd_probe(g.h, C.byref(probe(FAR | PQUAD))) == INVALID_ARG      # modifiers alone
    assert g.lib.psamd_potential(g.h, C.byref(pot(PQ | 0x4))) == INVALID_ARG
    assert g.lib.psamd_probe(g.h, C.byref(probe(A | FAR | PQUAD | 0x10))) == INVALID_ARG
    # no bit, or FAR alone: not this context's field
    for f in (0, ps.POTENTIAL_FAR):
        assert g.lib.psamd_potential(g.h, C.byref(pot(f))) == UNSUPPORTED
        assert g.lib.psamd_download_potential_flags(g.h, f, None, 0, None) == UNSUPPORTED
    assert g.lib.psamd_download_potential(g.h, None, 0, None) == UNSUPPORTED
    assert g.lib.psamd_download_potential_far(g.h, None, 0, None) == UNSUPPORTED
    for f in (A, P, A | P, A | FAR, A | P | FAR):
        assert g.lib.psamd_probe(g.h, C.byref(probe(f))) == UNSUPPORTED
    # both bits: served, with psamd_potential's and psamd_probe's arguments
    assert g.lib.psamd_potential(g.h, C.byref(pot(PQ, capacity=-1))) == INVALID_ARG
    assert g.lib.psamd_potential(g.h, C.byref(pot(PQ, reserved=1))) == INVALID_ARG
    assert g.lib.psamd_download_potential_flags(g.h, PQ, None, 5, None) == INVALID_ARG
    assert g.lib.psamd_download_potential_flags(g.h, PQ, None, -1, None) == INVALID_ARG
    assert g.lib.psamd_probe(g.h, C.byref(probe(A | FAR | PQUAD, 4))) == INVALID_ARG      # no arrays
    assert g.lib.psamd_potential(g.h, C.byref(pot(PQ))) == 0
    dev = torch.full((5,), 7, dtype=torch.int64, device=DEV)
    spec = probe(A | P | FAR | PQUAD)
    spec.result_dev = dev.data_ptr()
    assert g.lib.psamd_probe(g.h, C.byref(spec)) == 0                     # max_count == 0: a zero result
    g.synchronize()
    assert not dev.cpu().numpy().any() and not any(g.probe_result().values())
    r = ps.PotentialResult()
    assert g.lib.psamd_download_potential_flags(g.h, PQ, None, 0, C.byref(r)) == 0
    down = g.download_potential(far=True, quadrupole=True)
    assert r.to_dict() == record(down) == g.potential_result() and down["listed"] == len(down["phi"]) == 2000
    e = g.energy(far=True, quadrupole=True)
    assert e["potential"] == down["potential"] < 0 and e["total"] == e["kinetic"] + e["potential"]
    assert g.probe(pos4_of(c["xyz"][:64]), far=True, quadrupole=True)["served"] == 64
    g.calc_forces_pairs(); g.calc_forces_apply()
    assert g.lib.psamd_potential(g.h, C.byref(pot(PQ))) == STATE          # the frame has ended
    g.step(1); g.synchronize()                                            # the context steps on
    assert g.live_count() >= 1950
    g.close()
