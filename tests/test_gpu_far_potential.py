"""PSAMD_POTENTIAL_FAR and PSAMD_PROBE_FAR on the device (include/psamd.h, "energy" and "the field at chosen points", far-
monopole contexts): phi and U against the numpy model (far_model.py; 1e-5 relative, psamd_potential's bar), the
exact limits (a confined cloud: the cutoff context's bytes; G = 4: the flat context's), one adult per cell against an
all-pairs context, a list of two slices, the probe's acceleration against the force records BIT FOR BIT, the probe's phi,
the same bytes however the call is made, the refusals.

Contexts hold max_particles_num=16384 (far_harness.py's GRID): 4^3 (one level), 8^3 (8, 4), 10^3 (10, 5, 3: ragged)
and 16^3 (16, 8, 4: levels of several blocks)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import far_model as F
import particlesystem_amd as ps
from far_harness import GRID, INVALID_ARG, STATE, UNSUPPORTED, box_cloud, fill_lists, hip_runtime, low_corner, open_frame
from util import assert_same_particles

pytestmark = pytest.mark.gpu

PYR, MONO = ps.FLAG_FAR_PYRAMID, ps.FLAG_FAR_MONOPOLE
METHOD = {MONO: "flat", PYR: "pyramid"}                               # (far_model.py's names)
REL = 1e-5
EPS2 = 0.2
DEV = torch.device("cuda", 0)
BOTH = pytest.mark.parametrize("flag", [MONO, PYR], ids=["flat", "pyramid"])


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make(G, flags, **over):
    g = ps.ParticleSystem(ps.default_config(flags=flags, collision_radius=1e-6, **GRID[G], **over))
    assert g.sizes.grid_dim == G
    return g


def body_cloud(n, seed, G, kids=True):
    rng = np.random.default_rng(seed)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    if kids:
        age[::17] = 0.5                                                   # some kids: exert nothing, get the field at their own place
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


def scene(G, flag, sign=1.0):
    return _scene(int(G), int(flag), float(sign))


@functools.lru_cache(maxsize=None)
def _scene(G, flag, sign):
    """one frame of a cloud with kids on a far context, everything the tests below compare: the far phi (order of the fill) and
    its record, the model's fp64 phi, the force records (sorted order), the lists.  Computed once, never changed."""
    n = {8: 6000, 10: 8000, 16: 16384}[G]
    c = body_cloud(n, 40 + G, G)
    g = make(G, flag, force_sign=sign)
    ids = g.fill_particles(**c)
    open_frame(g)
    res = g.download_potential(far=True)
    lists, order = fill_lists(g, ids)
    assert len(order) == n and g.counters["cell_overflow_kills"] == 0
    g.calc_forces_pairs()
    f = g.download_force4(0, n)
    g.calc_forces_apply()
    g.close()
    kid = c["age"] < 1.5
    w_eff = np.where(kid, np.float32(0.0), np.float32(sign) * c["w"]).astype(np.float32)
    cell = F.cells_of(c["xyz"], G)
    moments = F.level_moments(lists, c["xyz"], w_eff, G, METHOD[flag])
    want = F.phi64(lists, c["xyz"], w_eff, G, EPS2, c["xyz"], cell, np.arange(n), METHOD[flag], moments)
    return dict(c=c, ids=ids, res=res, phi=by_fill(ids, res["phi"]), lists=lists, order=order, f=f, kid=kid, w_eff=w_eff, cell=cell,
                moments=moments, want=want)


# ---- 1. against the model -----------------------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("G,sign", [(8, 1.0), (8, -1.0), (10, 1.0), (16, 1.0), (16, -1.0)])
def test_phi_and_U_follow_the_model(G, sign, flag):
    """kids present (they are given the field at their own position); repulsion flips phi and U together"""
    s = scene(G, flag, sign)
    rel = np.abs(s["phi"].astype(np.float64) - s["want"]) / np.abs(s["want"])
    U = F.energy(s["w_eff"], s["want"])
    near = F.phi64(s["lists"], s["c"]["xyz"], s["w_eff"], G, EPS2, s["c"]["xyz"][:200], s["cell"][:200], np.arange(200), METHOD[flag], far=False)
    faith = F.phi32(s["lists"], s["c"]["xyz"], s["w_eff"], G, EPS2, s["c"]["xyz"][:400], s["cell"][:400], np.arange(400), METHOD[flag], s["moments"])
    rel32 = np.abs(s["phi"][:400].astype(np.float64) - faith) / np.abs(faith)
    print("far phi, %d bodies on %d^3 cells, flags %#x, sign %+.0f: max relative deviation from the model %.3g, U %.3g; from the "
          "model's fp32 association %.3g; the stencil alone is %.3g of phi (median)"
          % (len(rel), G, flag, sign, rel.max(), abs(s["res"]["potential"] - U) / abs(U), rel32.max(),
             np.median(near / s["want"][:200])))
    assert s["res"]["listed"] == len(rel) and s["res"]["nonfinite"] == 0 and s["kid"].sum() > 100
    assert (np.sign(s["want"]) == -sign).all() and np.median(near / s["want"][:200]) < 0.5      # (the far part is no small correction)
    assert rel.max() < REL
    assert abs(s["res"]["potential"] - U) < REL * abs(U)
    assert rel32.max() < F.ALLOW
    assert s["res"]["phi_min"] == float(s["phi"].min()) and s["res"]["phi_max"] == float(s["phi"].max())


# ---- 2., 3. the exact limits ------------------------------------------------------------------------------------------------

def test_confined_cloud_is_the_cutoff_result_byte_for_byte():
    """a cloud inside a 2x2x2 block of cells of the default 16^3 grid: no far body at any level"""
    n = 3000
    rng = np.random.default_rng(7)
    xyz = rng.uniform(-4.99, 4.99, (n, 3)).astype(np.float32)
    age = rng.uniform(0.5, 7.5, n).astype(np.float32)
    got = []
    for flags in (0, MONO, PYR):
        g = ps.ParticleSystem(ps.default_config(flags=flags))
        g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
        open_frame(g)
        got.append(g.potential(phi=True, far=flags != 0))
        got.append(g.download_potential(far=flags != 0))
        g.calc_forces()
        g.close()
    assert got[0]["listed"] == n and got[0]["potential"] < 0
    for r in got[1:]:
        assert np.array_equal(bits(r["phi"]), bits(got[0]["phi"])) and record(r) == record(got[0])


def test_one_level_is_the_flat_context_byte_for_byte():
    c = body_cloud(2048, 81, 4)
    got = []
    for flag in (PYR, MONO):
        g = make(4, flag)
        g.fill_particles(**c)
        open_frame(g)
        got.append(g.potential(phi=True, far=True))
        near = g.probe(pos4_of(c["xyz"]), far=True)
        got.append(near["out4"])
        g.calc_forces()
        g.close()
    assert got[0]["listed"] == 2048 and np.array_equal(bits(got[0]["phi"]), bits(got[2]["phi"])) and record(got[0]) == record(got[2])
    assert np.array_equal(bits(got[1]), bits(got[3]))
    s = np.abs(got[0]["phi"].cpu().numpy())
    assert s.min() > 0


# ---- 4. one adult per cell ------------------------------------------------------------------------------------------------

def test_one_adult_per_cell_is_the_all_pairs_phi():
    """at most one adult (and some kids) a cell: the cells' monopoles ARE the adults, every far body of the flat method is
    exact.  (Not so for the pyramid, whose coarser levels merge adults: it has no such limit.)"""
    G, flag = 8, MONO
    rng = np.random.default_rng(91)
    cells = rng.choice(G ** 3, 300, replace=False)
    i3, rem = np.divmod(cells, G * G)
    i1, i2 = np.divmod(rem, G)
    xyz = np.array([low_corner(a, b, c, G) for a, b, c in zip(i1, i2, i3)]) + rng.uniform(0.1, 4.9, (300, 3))
    kids = xyz[:40] + rng.uniform(-0.05, 0.05, (40, 3))
    xyz = np.concatenate([xyz, kids]).astype(np.float32)
    age = np.concatenate([np.full(300, 3.0), np.full(40, 0.5)]).astype(np.float32)
    w = rng.uniform(20.0, 100.0, 340).astype(np.float32)
    got = []
    for flags in (flag, ps.FLAG_ALL_PAIRS):
        g = make(G, flags)
        g.fill_particles(xyz, age=age, w=w, fert_age=np.float32(1e6))
        open_frame(g)
        got.append(g.download_potential(far=flags == flag))
        g.calc_forces()
        g.close()
    a, b = got[0]["phi"].astype(np.float64), got[1]["phi"].astype(np.float64)
    rel = np.abs(a - b) / np.abs(b)
    print("one adult a cell, flags %#x: far phi against the all-pairs context's, max %.3g; U %.3g"
          % (flag, rel.max(), abs(got[0]["potential"] - got[1]["potential"]) / abs(got[1]["potential"])))
    assert got[0]["listed"] == got[1]["listed"] == 340
    assert rel.max() < REL and abs(got[0]["potential"] - got[1]["potential"]) < REL * abs(got[1]["potential"])


# ---- 5. a list of two slices ------------------------------------------------------------------------------------------------

@BOTH
def test_both_slices_of_a_long_list_carry_the_far_part(flag):
    G = 8
    g = make(G, flag)
    many = g.sizes.max_per_cell                                           # a full list: 64 lanes and a ragged second slice
    assert 64 < many < 128
    c = body_cloud(3000, 95, G)
    rng = np.random.default_rng(96)
    crowd = (low_corner(4, 2, 3, G) + rng.uniform(0.05, 4.95, (many, 3))).astype(np.float32)
    full = (3 * G + 4) * G + 2
    keep = F.cells_of(c["xyz"], G) != full
    xyz = np.concatenate([c["xyz"][keep], crowd])
    age = np.concatenate([c["age"][keep], np.full(many, 3.0, np.float32)])
    w = np.concatenate([c["w"][keep], np.full(many, 60.0, np.float32)])
    ids = g.fill_particles(xyz, age=age, w=w, fert_age=np.float32(1e6))
    open_frame(g)
    res = g.potential(phi=True, far=True)
    ex = g.export_live(ps.EXPORT_ID | ps.EXPORT_POS)
    lists, _ = fill_lists(g, ids)
    g.calc_forces()
    kills = g.counters["cell_overflow_kills"]
    g.close()
    assert len(lists[full]) == many and kills == 0
    assert np.array_equal(ex["id"].cpu().numpy(), np.sort(ids)) and len(res["phi"]) == len(ids)
    where = np.full(ids.max() + 1, -1)
    where[ids] = np.arange(len(ids))
    assert np.array_equal(ex["pos4"].cpu().numpy()[:, :3], xyz[where[ex["id"].cpu().numpy()]])      # entry for entry with the export
    phi = by_fill(ids, res["phi"])
    w_eff = np.where(age < 1.5, np.float32(0), w).astype(np.float32)
    crowd_idx = lists[full]
    cell = np.full(many, full)
    want = F.phi64(lists, xyz, w_eff, G, EPS2, xyz[crowd_idx], cell, crowd_idx, METHOD[flag])
    near = F.phi64(lists, xyz, w_eff, G, EPS2, xyz[crowd_idx], cell, crowd_idx, METHOD[flag], far=False)
    rel = np.abs(phi[crowd_idx] - want) / np.abs(want)
    print("a list of %d, flags %#x: max relative deviation %.3g (first slice %.3g, second %.3g); far part %.3g of phi"
          % (many, flag, rel.max(), rel[:64].max(), rel[64:].max(), np.median(1 - near / want)))
    assert rel.max() < REL and np.median(1 - near / want) > 100 * REL    # (a slice without its far part would miss by that much)


# ---- 6. the probe repeats the force record ------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,flag", [(8, MONO), (16, MONO), (10, PYR), (16, PYR)], ids=["flat-8", "flat-16", "pyramid-10", "pyramid-16"])
def test_an_acc_probe_on_a_served_adult_is_its_force_record_bit_for_bit(G, flag):
    """8^3 flat: 8 blocks over 16 parts; 16^3: 64 blocks, 4 a part, and as a pyramid level 0 of 64 blocks and level 1 of 8.
    At 16^3 there are 4 bodies a cell: a wave of 64 probes sits in some 16 cells under several parents"""
    s = scene(G, flag)
    g = make(G, flag)
    g.fill_particles(**s["c"])
    open_frame(g)
    adults = s["order"][~s["kid"][s["order"]]]
    out = g.probe(pos4_of(s["c"]["xyz"][adults]), phi=False, far=True)
    g.calc_forces()
    g.close()
    f = s["f"][~s["kid"][s["order"]]]
    assert (f[:, 3].view(np.int32) == 0).all() and np.abs(f[:, :3]).max() > 0      # (every adult was served: no collision)
    got = out["out4"].cpu().numpy()
    assert out["served"] == len(adults) and out["nonfinite"] == 0 and not got[:, 3].any()
    if G == 16:
        first = s["cell"][adults[:64]]                                    # (sorted order: cell-major, as the probes are served)
        i1, i2, i3 = (first // G % G) >> 1, (first % G) >> 1, (first // (G * G)) >> 1
        assert len(np.unique(first)) >= 8 and len(np.unique((i3 * 8 + i1) * 8 + i2)) >= 2      # one wave: many cells, more than one parent
    bad = np.nonzero((bits(got[:, :3]) != bits(f[:, :3])).any(1))[0]
    assert len(bad) == 0, "%d of %d probes differ from the force record, first %d: probe %r record %r" % (len(bad), len(adults), bad[0], got[bad[0]], f[bad[0]])


@BOTH
def test_fast_math_probes_give_the_same_bytes_twice_and_follow_the_model(flag):
    G = 8
    s = scene(G, flag)
    adults = np.nonzero(~s["kid"])[0][:2000]
    outs = []
    for _ in range(2):
        g = make(G, flag | ps.FLAG_FAST_MATH)
        g.fill_particles(**s["c"])
        open_frame(g)
        outs.append(g.probe(pos4_of(s["c"]["xyz"][adults]), far=True)["out4"].cpu().numpy())
        g.calc_forces()
        g.close()
    assert outs[0].tobytes() == outs[1].tobytes()
    want = F.accel64(s["lists"], s["c"]["xyz"], s["w_eff"], G, EPS2, s["c"]["xyz"][adults], s["cell"][adults], METHOD[flag], s["moments"])
    rel = F.rel_dev(outs[0][:, :3].astype(np.float64), want)
    print("fast-math far probes, flags %#x: max relative deviation of a from the model %.3g" % (flag, rel.max()))
    assert rel.max() < REL


# ---- 7. the probe's phi ---------------------------------------------------------------------------------------------------

@BOTH
@pytest.mark.parametrize("G", [8, 16])
def test_probe_phi(G, flag):
    s = scene(G, flag)
    c, n = s["c"], len(s["ids"])
    g = make(G, flag)
    g.fill_particles(**c)
    open_frame(g)
    on = g.probe(pos4_of(c["xyz"]), acc=False, far=True)["out4"].cpu().numpy()[:, 3]
    # a regular grid of points, two of them outside the box and one not a number
    k = np.arange(12)
    half = G * 2.5
    grid = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3) * (2 * half / 12) - half + 0.37
    grid = np.concatenate([grid, [[half + 1.0, 0, 0], [0, -half - 3.0, 0], [np.nan, 0, 0]]]).astype(np.float32)
    res = g.probe(pos4_of(grid), far=True, outcome=True)
    g.calc_forces()
    g.close()
    kid = s["kid"]
    assert np.array_equal(bits(on[kid]), bits(s["phi"][kid]))             # a kid's true position: its far phi, bit for bit
    own = -(s["w_eff"][~kid].astype(np.float64)) / np.sqrt(np.float64(np.float32(EPS2)))
    rel = np.abs(on[~kid] - (s["phi"][~kid].astype(np.float64) + own)) / np.abs(on[~kid])
    out4, code = res["out4"].cpu().numpy(), res["outcome"].cpu().numpy()
    assert code[-3:].tolist() == [ps.PROBE_OUTSIDE] * 3 and (bits(out4[-3:]) == 0x7fc00000).all() and (code[:-3] == ps.PROBE_SERVED).all()
    assert res["served"] == 12 ** 3 and res["outside"] == 3 and res["nonfinite"] == 0
    cell = F.cells_of(grid[:-3], G)
    minus = np.full(len(cell), -1)
    want = F.phi64(s["lists"], c["xyz"], s["w_eff"], G, EPS2, grid[:-3], cell, minus, METHOD[flag], s["moments"])
    wacc = F.accel64(s["lists"], c["xyz"], s["w_eff"], G, EPS2, grid[:-3], cell, METHOD[flag], s["moments"])
    rphi = np.abs(out4[:-3, 3] - want) / np.abs(want)
    racc = F.rel_dev(out4[:-3, :3].astype(np.float64), wacc)
    print("far probes on %d^3 cells, flags %#x: on adults, phi + own term to %.3g; on a grid phi to %.3g, a to %.3g"
          % (G, flag, rel.max(), rphi.max(), racc.max()))
    assert rel.max() < 4 * 2.0 ** -24                                     # two roundings to fp32 and the sum's: "to rounding"
    assert rphi.max() < REL and racc.max() < REL


# ---- 8. the same bytes however it is called -------------------------------------------------------------------------------------

@BOTH
def test_the_same_bytes_before_and_after_the_pair_stage_and_nothing_else_moves(flag):
    G = 8
    s = scene(G, flag)
    g = make(G, flag)
    b = make(G, flag)                                                     # never makes a far call
    for x in (g, b):
        x.fill_particles(**s["c"])
        open_frame(x)
    pts = pos4_of(s["c"]["xyz"][:1000])
    first = g.potential(phi=True, far=True)
    again = g.potential(phi=True, far=True)
    p1 = g.probe(pts, far=True)["out4"]
    g.calc_forces_pairs(); b.calc_forces_pairs()
    after = g.download_potential(far=True)
    p2 = g.probe(pts, far=True)["out4"]
    n = len(s["ids"])
    fa, fb = g.download_force4(0, n), b.download_force4(0, n)
    mom = [x.download_level_moments(0) if flag == PYR else x.download_cell_moments() for x in (g, b)]
    g.calc_forces_apply(); b.calc_forces_apply()
    g.step(1); b.step(1)
    for r in (again, after):
        assert np.array_equal(bits(r["phi"]), bits(first["phi"])) and record(r) == record(first)
    assert np.array_equal(bits(first["phi"]), bits(s["res"]["phi"])) and np.array_equal(bits(p1), bits(p2))
    assert fa.tobytes() == fb.tobytes() == s["f"].tobytes() and mom[0].tobytes() == mom[1].tobytes()
    assert_same_particles(g.download_particles(), b.download_particles(), "a step after far potential calls")
    assert g.counters == b.counters
    g.close(); b.close()


@BOTH
def test_the_far_call_is_captured_into_a_graph_and_replays_on_a_later_frame(flag):
    G = 8
    g = make(G, flag)
    c = body_cloud(6000, 48, G)
    g.fill_particles(**c, vxyz=box_cloud(6000, 49, 2.0))
    g.step(1)
    open_frame(g)
    cap = g.owned_slots()
    phi = torch.zeros(cap, dtype=torch.float32, device=DEV)
    rec = torch.zeros(C.sizeof(ps.PotentialResult), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    spec = ps.Potential(flags=ps.POTENTIAL_FAR, phi=phi.data_ptr(), capacity=cap, result_dev=rec.data_ptr())
    hip = hip_runtime()
    stream = C.c_void_p(g.stream())
    graph, exe = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 2) == 0                      # hipStreamCaptureModeRelaxed
    rc = g.lib.psamd_potential(g.h, C.byref(spec))
    assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and rc == 0
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
    g.calc_forces()
    g.step(2)
    open_frame(g)                                                         # another frame: the graph holds nothing of the one it was captured in
    assert hip.hipGraphLaunch(exe, stream) == 0
    assert hip.hipStreamSynchronize(stream) == 0
    replayed = ps.PotentialResult.from_buffer_copy(rec.cpu().numpy().tobytes()).to_dict()
    eager = g.potential(phi=True, far=True)
    assert replayed == record(eager) == g.potential_result()
    assert replayed["listed"] == len(eager["phi"]) > 0
    assert np.array_equal(bits(phi[:len(eager["phi"])]), bits(eager["phi"]))
    assert hip.hipGraphExecDestroy(exe) == 0 and hip.hipGraphDestroy(graph) == 0
    g.calc_forces()
    g.synchronize()
    g.close()


# ---- 9. refusals and arguments ----------------------------------------------------------------------------------------------

def test_refusals_and_arguments():
    c = body_cloud(2000, 71, 8)
    far_spec = ps.Potential(flags=ps.POTENTIAL_FAR)
    probe = lambda fields, m=0: ps.ProbeSpec(fields=fields, max_count=m)
    for flags in (0, ps.FLAG_ALL_PAIRS):                                  # the bits are unknown bits there
        g = make(8, flags)
        g.fill_particles(**c)
        open_frame(g)
        assert g.lib.psamd_potential(g.h, C.byref(far_spec)) == INVALID_ARG
        assert g.lib.psamd_probe(g.h, C.byref(probe(ps.PROBE_ACC | ps.PROBE_FAR))) == INVALID_ARG
        assert g.lib.psamd_download_potential_far(g.h, None, 0, None) == UNSUPPORTED
        assert g.download_potential(phi=False)["listed"] == 2000          # the context stayed usable
        g.calc_forces()
        g.close()
    for flag in (MONO, PYR):
        g = make(8, flag)
        g.fill_particles(**c)
        assert g.lib.psamd_potential(g.h, C.byref(far_spec)) == STATE    # outside the window
        assert g.lib.psamd_download_potential_far(g.h, None, 0, None) == STATE
        assert g.lib.psamd_probe(g.h, C.byref(probe(ps.PROBE_PHI | ps.PROBE_FAR))) == STATE
        open_frame(g)
        assert g.lib.psamd_potential(g.h, C.byref(ps.Potential())) == UNSUPPORTED      # without the bit: as before
        assert g.lib.psamd_download_potential(g.h, None, 0, None) == UNSUPPORTED
        assert g.lib.psamd_probe(g.h, C.byref(probe(ps.PROBE_ACC | ps.PROBE_PHI))) == UNSUPPORTED
        assert g.lib.psamd_probe(g.h, C.byref(probe(ps.PROBE_FAR))) == INVALID_ARG      # a modifier alone
        assert g.lib.psamd_probe(g.h, C.byref(probe(ps.PROBE_ACC | ps.PROBE_FAR | 0x8))) == INVALID_ARG
        assert g.lib.psamd_potential(g.h, C.byref(ps.Potential(flags=ps.POTENTIAL_FAR | 0x2))) == INVALID_ARG
        assert g.lib.psamd_potential(g.h, C.byref(ps.Potential(flags=ps.POTENTIAL_FAR, capacity=-1))) == INVALID_ARG
        assert g.lib.psamd_download_potential_far(g.h, None, 5, None) == INVALID_ARG
        assert g.lib.psamd_probe(g.h, C.byref(probe(ps.PROBE_ACC | ps.PROBE_FAR, 4))) == INVALID_ARG      # no arrays
        dev = torch.full((5,), 7, dtype=torch.int64, device=DEV)
        spec = probe(ps.PROBE_ACC | ps.PROBE_PHI | ps.PROBE_FAR)
        spec.result_dev = dev.data_ptr()
        assert g.lib.psamd_probe(g.h, C.byref(spec)) == 0                 # max_count == 0: a zero result
        g.synchronize()
        assert not dev.cpu().numpy().any() and not any(g.probe_result().values())
        assert g.energy(far=True)["potential"] == g.download_potential(phi=False, far=True)["potential"] < 0
        g.calc_forces_pairs(); g.calc_forces_apply()
        assert g.lib.psamd_potential(g.h, C.byref(far_spec)) == STATE    # the frame has ended
        g.step(1); g.synchronize()
        assert g.live_count() >= 1950
        g.close()
