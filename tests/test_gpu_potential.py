"""Potential energy and per-particle potential on the device (psamd_potential / psamd_download_potential /
psamd_potential_result_get, potential.hip).

The reference value everywhere is an fp64 direct sum over the frame's bodies, formed here with numpy from the
downloaded fp32 positions, ages (the kid rule: age < KID_AGE has mass 0), masses and cell lists (download_cellgrid):
    phi_i = - s * sum over j != i (by id) of w_eff_j / sqrt(|x_j - x_i|^2 + eps2),   U = 1/2 sum_i w_eff_i phi_i
over the 27-cell non-periodic stencil of i's cell (every listed body of the box for an all-pairs context).  The bound
on phi and on U is 1e-5 relative, the project's bound for arithmetic the reference cannot pin (BASELINE north_star,
tests/test_gpu_extras.py); masses are non-negative, so nothing cancels and the bound on U follows from the one on phi.

Slabs: a plane group is the cell layers {kD - 1, kD} (partition.hpp), so on the default 16^3 grid (chunk_dim D = 4) the
group-aligned cuts, which lend nothing, fall at kD - 1: [0, 7, 16] and [0, 3, 7, 11, 16] are the byte-equality cases
(worlds 2 and 4).  A cut at a multiple of chunk_dim falls inside a plane group and lends layer kD: [0, 8, 16] is the
refusal case."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import particlesystem_amd as ps
from particlesystem_amd import slab
from service_harness import ERR_INVALID_ARG, ERR_STATE, ERR_UNSUPPORTED, bits, captured, kid_age, open_frame, slab_inputs
from util import SENTINEL, capacities, cloud, ragged

pytestmark = pytest.mark.gpu

REL = 1e-5
SMALL = dict(chunk_factor=2, chunk_dim=4)          # an 8^3 grid of 5-unit cells: the box is [-20, 20)^3


def by_id(g, res=None, capacity=None):
    """phi of this point of the stream by global slot id (float32 array over the container, NaN elsewhere), the ids"""
    res = g.potential(phi=True, capacity=capacity) if res is None else res
    ex = g.export_live(ps.EXPORT_ID, capacity=capacity)
    ids = ex["id"].cpu().numpy()
    assert len(ids) == len(res["phi"])
    out = np.full(g.sizes.container_size, np.nan, np.float32)
    out[ids] = res["phi"].cpu().numpy()
    return out, ids, res


class Frame:
    """what the reference sum needs of a built frame, downloaded"""

    def __init__(self, g, p=None, cg=None):
        p = g.download_particles() if p is None else p
        cg = g.download_cellgrid() if cg is None else cg
        self.G, self.eps2 = g.sizes.grid_dim, float(g.cfg.eps2)
        self.s = -1.0 if g.cfg.force_sign < 0 else 1.0
        self.xyz = np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float64)
        self.w = np.where(p["age"].astype(np.float64) < kid_age(g.cfg), 0.0, p["w"].astype(np.float64))
        self.count = cg[:, 0].astype(np.int64)
        self.lists = cg[:, 1:]
        self.listed = np.concatenate([self.lists[c, :self.count[c]] for c in np.nonzero(self.count)[0]] or [np.zeros(0, np.int32)])

    def stencil_ids(self, c):
        G = self.G
        i3, r = divmod(int(c), G * G)
        i1, i2 = divmod(r, G)
        out = []
        for d3 in (-1, 0, 1):
            for d1 in (-1, 0, 1):
                for d2 in (-1, 0, 1):
                    j3, j1, j2 = i3 + d3, i1 + d1, i2 + d2
                    if 0 <= j3 < G and 0 <= j1 < G and 0 <= j2 < G:
                        n = (j3 * G + j1) * G + j2
                        out.append(self.lists[n, :self.count[n]])
        return np.concatenate(out)

    def phi_of(self, ids_i, ids_j):
        """fp64 direct sum for the particles ids_i over the bodies ids_j (self left out by id, kids add nothing)"""
        ids_j = ids_j[self.w[ids_j] != 0.0]
        out = np.empty(len(ids_i))
        rows = max(1, min(256, 2000000 // max(1, len(ids_j))))
        for a in range(0, len(ids_i), rows):
            ii = ids_i[a:a + rows]
            d = self.xyz[ids_j][None, :, :] - self.xyz[ii][:, None, :]
            t = self.w[ids_j][None, :] / np.sqrt((d * d).sum(-1) + self.eps2)
            t[ii[:, None] == ids_j[None, :]] = 0.0
            out[a:a + rows] = -self.s * t.sum(1)
        return out

    def phi_cutoff(self):
        """phi of every listed particle by slot id (NaN: not listed)"""
        phi = np.full(len(self.xyz), np.nan)
        for c in np.nonzero(self.count)[0]:
            ids_i = self.lists[c, :self.count[c]]
            phi[ids_i] = self.phi_of(ids_i, self.stencil_ids(c))
        return phi

    def energy(self, phi):
        ok = np.isfinite(phi[self.listed])
        ids = self.listed[ok]
        return 0.5 * float((self.w[ids] * phi[ids]).sum()), int((~ok).sum())


def check_against(fr, got_phi, res, ref_phi, what):
    """every listed particle's phi and U within REL of the reference; the counts; prints the largest error"""
    ids = fr.listed
    ref, got = ref_phi[ids], got_phi[ids].astype(np.float64)
    fin = np.isfinite(ref)
    assert not np.isfinite(got[~fin]).any(), what + ": a particle whose reference phi is not finite has a finite phi"
    assert np.isfinite(got[fin]).all(), what + ": a particle has no finite phi though the reference has"
    err = np.abs(got[fin] - ref[fin]) / np.abs(ref[fin]) if fin.any() else np.zeros(1)
    u_ref, nonfinite = fr.energy(ref_phi)
    u_err = abs(res["potential"] - u_ref) / abs(u_ref) if u_ref != 0 else abs(res["potential"])
    print("%s: %d listed, largest relative error of phi %.3g, of U %.3g (U = %.9g)" % (what, len(ids), err.max(), u_err, res["potential"]))
    assert res["listed"] == len(ids) and res["nonfinite"] == nonfinite, (what, res, len(ids), nonfinite)
    assert err.max() <= REL, (what, err.max())
    assert u_err <= REL, (what, res["potential"], u_ref)
    if fin.any():
        assert res["phi_min"] == float(got[fin].min()) and res["phi_max"] == float(got[fin].max()), (what, res)
    return err.max(), u_err


def pair_system(extra=(), **over):
    """two adults of weight 60 in one cell, 1.5 apart, and whatever else"""
    g = ps.ParticleSystem(ps.default_config(**over))
    xyz = np.array([(1.0, 1.0, 1.0), (2.5, 1.0, 1.0)] + [e[0] for e in extra], np.float32)
    age = np.array([3.0, 3.0] + [e[1] for e in extra], np.float32)
    ids = g.fill_particles(xyz, age=age, fert_age=np.float32(1e6))
    open_frame(g)
    return g, ids


# ---- closed forms ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_two_adults_closed_form(sign):
    g, ids = pair_system(force_sign=sign)
    w, d, eps2 = 60.0, 1.5, g.cfg.eps2
    want = -sign * w / np.sqrt(d * d + eps2)
    phi, _, res = by_id(g)
    assert np.allclose(phi[ids].astype(np.float64), want, rtol=REL, atol=0), (phi[ids], want)
    assert abs(res["potential"] - w * want) <= REL * abs(w * want), (res, w * want)
    assert res["listed"] == 2 and res["nonfinite"] == 0
    assert res["phi_min"] == res["phi_max"] == float(phi[ids[0]]) and phi[ids[0]] == phi[ids[1]]
    assert (want < 0) == (sign > 0)
    g.close()


def test_a_kid_changes_nothing_and_gets_the_adults_potential():
    g, ids = pair_system()
    phi0, _, res0 = by_id(g)
    g.close()
    g, ids2 = pair_system(extra=[((1.0, 3.0, 1.0), 0.5)])       # age 0.5 < KID_AGE 1.5, 2 above the first adult
    assert 0.5 < kid_age(g.cfg) < 3.0
    phi, _, res = by_id(g)
    assert np.array_equal(bits(phi[ids2[:2]]), bits(phi0[ids])), "the kid changed an adult's phi"
    assert res["potential"] == res0["potential"] and res["listed"] == 3
    w, eps2 = 60.0, g.cfg.eps2
    want = -w / np.sqrt(4.0 + eps2) - w / np.sqrt(1.5 * 1.5 + 4.0 + eps2)
    assert abs(float(phi[ids2[2]]) - want) <= REL * abs(want), (phi[ids2[2]], want)
    g.close()


def test_a_particle_on_top_of_an_adult_is_seen_at_the_softening_length():
    g, ids = pair_system()
    phi0, _, _ = by_id(g)
    g.close()
    g, ids2 = pair_system(extra=[((1.0, 1.0, 1.0), 3.0)])       # exactly on the first adult: left out by index, not by distance
    phi, _, res = by_id(g)
    w, eps2 = 60.0, g.cfg.eps2
    far = -w / np.sqrt(1.5 * 1.5 + eps2)
    for k, want in ((0, far - w / np.sqrt(eps2)), (2, far - w / np.sqrt(eps2)), (1, 2 * far)):
        assert abs(float(phi[ids2[k]]) - want) <= REL * abs(want), (k, phi[ids2[k]], want)
    assert abs((float(phi[ids2[0]]) - float(phi0[ids[0]])) - (-w / np.sqrt(eps2))) <= REL * w / np.sqrt(eps2)
    assert res["listed"] == 3 and res["nonfinite"] == 0
    g.close()


# ---- accuracy ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per_cell", [4, 32, 256])
def test_uniform_cloud_against_the_fp64_direct_sum(per_cell):
    n = 512 * per_cell
    g = ps.ParticleSystem(ps.default_config(max_particles_num=2 * n, **SMALL))      # (lists twice the mean and more: nothing overflows)
    rng = np.random.default_rng(per_cell)
    age = rng.uniform(0.2, 9.0, n).astype(np.float32)            # one in seven is a kid
    w = rng.uniform(20.0, 100.0, n).astype(np.float32)
    g.fill_particles(cloud(n, 40 + per_cell, 20.0), age=age, w=w, fert_age=np.float32(1e6))
    open_frame(g)
    phi, ids, res = by_id(g)
    fr = Frame(g)
    assert res["listed"] == g.live_count() == len(ids) == n
    assert abs(fr.count.mean() - per_cell) < 1e-9 and fr.count.max() <= g.sizes.max_per_cell
    check_against(fr, phi, res, fr.phi_cutoff(), "uniform cloud, about %d per cell" % per_cell)
    # the numpy form is the same pass
    d = g.download_potential()
    assert np.array_equal(bits(d["phi"]), bits(res["phi"])) and {k: d[k] for k in res if k != "phi"} == {k: res[k] for k in res if k != "phi"}
    assert g.potential_result() == {k: res[k] for k in res if k != "phi"}
    g.close()


def test_clump_that_fills_cells_to_their_capacity():
    g = ps.ParticleSystem(ps.default_config(max_particles_num=1 << 18))
    cap = g.sizes.max_per_cell                                  # 130
    rng = np.random.default_rng(5)
    corner = np.array([(i2 * 5.0, -i1 * 5.0 - 5.0, -i3 * 5.0 - 5.0) for i3 in (0, 1) for i1 in (0, 1) for i2 in (0, 1)])    # low corners of a 2x2x2 block of cells
    clump = np.concatenate([c + rng.uniform(0.05, 4.95, (cap + 6, 3)) for c in corner])      # six more than each list holds
    xyz = np.concatenate([clump, cloud(3000, 6)]).astype(np.float32)
    g.fill_particles(xyz, age=np.float32(3.0), fert_age=np.float32(1e6))
    open_frame(g)
    phi, ids, res = by_id(g)
    fr = Frame(g)
    assert (fr.count == cap).sum() >= 8 and g.counters["cell_overflow_kills"] >= 48
    assert res["listed"] == g.live_count() == len(fr.listed)
    check_against(fr, phi, res, fr.phi_cutoff(), "clump at the list capacity %d" % cap)
    g.close()


# ---- alignment with the export ------------------------------------------------------------------------------------------

def test_phi_pairs_with_the_export_entry_for_entry():
    n = 20000
    g = ps.ParticleSystem(ps.default_config())
    xyz = cloud(n, 7)
    g.fill_particles(xyz, age=np.float32(3.0), fert_age=np.float32(1e6), vxyz=cloud(n, 8, 30.0))
    g.step(3)                                                   # collisions free slots: the live ids are no longer 0..n-1 in fill order
    open_frame(g)
    res = g.potential(phi=True)
    ex = g.export_live(ps.EXPORT_ID | ps.EXPORT_POS)
    live = g.live_count()
    assert ex["count"] == live == res["listed"] == len(res["phi"]) < n
    ids = ex["id"].cpu().numpy()
    assert (np.diff(ids) > 0).all()
    fr = Frame(g)
    p = g.download_particles()
    assert np.array_equal(ex["pos4"].cpu().numpy()[:, 0], p["x"][ids])
    full = np.full(g.sizes.container_size, np.nan, np.float32)
    full[ids] = res["phi"].cpu().numpy()
    check_against(fr, full, res, fr.phi_cutoff(), "stepped cloud")
    # a capacity smaller than the count truncates both alike
    cap = live // 3
    short, ex_short = g.potential(phi=True, capacity=cap), g.export_live(ps.EXPORT_ID, capacity=cap)
    assert len(short["phi"]) == cap == len(ex_short["id"])
    assert np.array_equal(bits(short["phi"]), bits(res["phi"][:cap])) and np.array_equal(ex_short["id"].cpu().numpy(), ids[:cap])
    assert {k: short[k] for k in short if k != "phi"} == {k: res[k] for k in res if k != "phi"}
    g.close()


# ---- determinism ----------------------------------------------------------------------------------------------------

def stepped(graphs, steps=4, n=60000):
    g = ps.ParticleSystem(ps.default_config())
    g.set_graphs(graphs)
    g.fill_particles(cloud(n, 21), age=np.float32(3.0), fert_age=np.float32(1e6), vxyz=cloud(n, 22, 20.0))
    g.step(steps)
    open_frame(g)
    return g


def test_same_bits_twice_with_graphs_and_after_the_pair_stage():
    g = stepped(False)
    a, b = g.potential(phi=True), g.potential(phi=True)
    assert np.array_equal(bits(a["phi"]), bits(b["phi"]))
    plain = {k: a[k] for k in a if k != "phi"}
    assert plain == {k: b[k] for k in b if k != "phi"} and C.c_double(a["potential"]).value == b["potential"]
    g.calc_forces_pairs()
    c = g.potential(phi=True)
    assert np.array_equal(bits(a["phi"]), bits(c["phi"])) and plain == {k: c[k] for k in c if k != "phi"}
    g.calc_forces_apply()
    h = stepped(True)
    d = h.potential(phi=True)
    assert h.graph_stats()[0] > 0
    assert np.array_equal(bits(a["phi"]), bits(d["phi"])) and plain == {k: d[k] for k in d if k != "phi"}
    g.close(); h.close()


def test_the_call_is_captured_into_a_graph_and_replays_on_a_later_frame():
    g = stepped(False, steps=2, n=30000)
    dev = torch.device("cuda", 0)
    cap = g.owned_slots()
    phi = torch.zeros(cap, dtype=torch.float32, device=dev)
    rec = torch.zeros(C.sizeof(ps.PotentialResult), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    spec = ps.Potential(phi=phi.data_ptr(), capacity=cap, result_dev=rec.data_ptr())
    with captured(g) as cap:
        rc = g.lib.psamd_potential(g.h, C.byref(spec))
    assert rc == 0
    g.calc_forces()
    g.step(2)
    open_frame(g)                                                    # another frame: the graph holds nothing of the one it was captured in
    cap.launch()
    replayed = ps.PotentialResult.from_buffer_copy(rec.cpu().numpy().tobytes()).to_dict()
    eager = g.potential(phi=True)
    assert replayed == {k: eager[k] for k in eager if k != "phi"} == g.potential_result()
    assert replayed["listed"] == len(eager["phi"]) > 0
    assert np.array_equal(bits(phi[:len(eager["phi"])]), bits(eager["phi"]))
    cap.close()
    g.calc_forces()
    g.synchronize()
    g.close()


# ---- all-pairs ------------------------------------------------------------------------------------------------------

def test_all_pairs_cloud_inside_a_block_of_cells_is_the_cutoff_result():
    rng = np.random.default_rng(31)
    xyz = rng.uniform((0.1, -9.9, -9.9), (9.9, -0.1, -0.1), (3000, 3)).astype(np.float32)      # a 2x2x2 block of cells
    got = []
    for flags in (0, ps.FLAG_ALL_PAIRS):
        g = ps.ParticleSystem(ps.default_config(max_particles_num=1 << 18, flags=flags))
        g.fill_particles(xyz, age=np.float32(3.0), fert_age=np.float32(1e6))
        open_frame(g)
        got.append(g.potential(phi=True))
        assert (Frame(g).count > 0).sum() == 8
        g.close()
    assert np.array_equal(bits(got[0]["phi"]), bits(got[1]["phi"]))
    assert {k: got[0][k] for k in got[0] if k != "phi"} == {k: got[1][k] for k in got[1] if k != "phi"}


def direct_energy(xyz, w, eps2, workers=16):
    """U = -sum over pairs i < j of w_i w_j / sqrt(r^2 + eps2), fp64, in blocks (numpy releases the GIL inside them)"""
    n, B, W = len(xyz), 512, 2048
    cols = [np.ascontiguousarray(xyz[:, k]) for k in range(3)]

    def block(a):
        rows = slice(a, min(a + B, n))
        s = 0.0
        for b in range(a, n, W):
            col = slice(b, min(b + W, n))
            r2 = np.full((rows.stop - rows.start, col.stop - col.start), eps2)
            for k in range(3):
                d = cols[k][col][None, :] - cols[k][rows][:, None]
                d *= d
                r2 += d
            np.sqrt(r2, out=r2)
            np.divide(w[col][None, :], r2, out=r2)
            if b < rows.stop:                  # the block holds the diagonal: pairs j > i only
                jj, ii = np.arange(col.start, col.stop)[None, :], np.arange(rows.start, rows.stop)[:, None]
                r2[jj <= ii] = 0.0
            s += float(w[rows] @ r2.sum(1))
        return s
    with ThreadPoolExecutor(workers) as ex:
        return -sum(ex.map(block, range(0, n, B)))


def test_all_pairs_spread_cloud_against_the_fp64_direct_sum():
    n = 1 << 18                                                 # BASELINE configs[1]
    g = ps.ParticleSystem(ps.default_config(max_particles_num=n, flags=ps.FLAG_ALL_PAIRS))
    w = np.random.default_rng(32).uniform(20.0, 100.0, n).astype(np.float32)
    g.fill_particles(cloud(n, 33), age=np.float32(3.0), w=w, fert_age=np.float32(1e6))
    open_frame(g)
    phi, ids, res = by_id(g)
    fr = Frame(g)
    assert res["listed"] == n == len(fr.listed) and res["nonfinite"] == 0
    sample = np.sort(np.random.default_rng(34).choice(fr.listed, 4096, replace=False))
    ref = fr.phi_of(sample, fr.listed)
    err = np.abs(phi[sample].astype(np.float64) - ref) / np.abs(ref)
    u_ref = direct_energy(fr.xyz[fr.listed], fr.w[fr.listed], fr.eps2)
    u_err = abs(res["potential"] - u_ref) / abs(u_ref)
    print("all-pairs N = 2^18: largest relative error of phi over the sample %.3g, of U %.3g (U = %.12g)" % (err.max(), u_err, res["potential"]))
    assert err.max() <= REL and u_err <= REL
    g.close()


# ---- a particle that is no number -------------------------------------------------------------------------------------------

def test_a_particle_whose_position_is_no_number():
    n = 30000
    g = ps.ParticleSystem(ps.default_config())
    g.fill_particles(cloud(n, 51), age=np.float32(3.0), fert_age=np.float32(1e6))
    p = g.download_particles()
    victim = int(np.nonzero(p["cell"] == 0)[0][0])              # cell 0 is where the reference files such a position (grid.hip, k_unpack_aos)
    p["x"][victim] = p["y"][victim] = p["z"][victim] = np.nan
    g.upload_particles(p)
    open_frame(g)
    phi, ids, res = by_id(g)
    fr = Frame(g)
    ref = fr.phi_cutoff()
    bad = ~np.isfinite(ref[fr.listed])
    assert 1 < bad.sum() < 200 and not np.isfinite(ref[victim])         # itself and everybody who has it in the stencil
    assert res["nonfinite"] == bad.sum() and res["listed"] == n
    assert not np.isfinite(phi[fr.listed[bad]]).any() and np.isfinite(phi[fr.listed[~bad]]).all()
    check_against(fr, phi, res, ref, "a NaN position among adults")
    g.calc_forces()                                              # nothing faulted: the step goes on
    g.synchronize()
    g.close()


# ---- slabs ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cuts,flags", [([0, 7, 16], 0), ([0, 3, 7, 11, 16], 0), ([0, 7, 16], ps.FLAG_ALL_PAIRS)])
def test_slabs_give_the_single_context_bytes(cuts, flags):
    xyz, age, v = slab_inputs(50000 if not flags else 20000, 61)
    over = dict(flags=flags, max_particles_num=1 << 18) if flags else dict(flags=flags)
    one = ps.ParticleSystem(ps.default_config(**over))
    one.fill_particles(xyz, age=age, fert_age=np.float32(1e6), vxyz=v)
    world = len(cuts) - 1
    ranks = [ps.ParticleSystem(ps.default_config(rank=r, world=world, cuts=cuts, **over)) for r in range(world)]
    for s in ranks:
        s.fill_particles(xyz, age=age, fert_age=np.float32(1e6), vxyz=v)
    for step in range(3):
        if step:
            one.step(1)
            slab.step_local(ranks)
        open_frame(one)
        want, ids, res = by_id(one)
        slab.to_pairs(ranks)
        union = np.full(one.sizes.container_size, np.nan, np.float32)
        parts, seen = [], 0
        for s in ranks:
            pl = s.slab_plan()
            assert pl.lentin_lo == pl.lentin_hi and pl.lentout_lo == pl.lentout_hi
            phi_r, ids_r, res_r = by_id(s)
            assert np.isnan(union[ids_r]).all()
            union[ids_r] = phi_r[ids_r]
            seen += len(ids_r)
            parts.append(res_r)
        assert seen == len(ids)
        assert np.array_equal(bits(union), bits(want)), "step %d: the ranks' phi differ from the single context's" % step
        merged = ps.merge_potential(parts)
        assert merged["listed"] == res["listed"] and merged["nonfinite"] == res["nonfinite"]
        assert merged["phi_min"] == res["phi_min"] and merged["phi_max"] == res["phi_max"]
        assert abs(merged["potential"] - res["potential"]) <= 1e-12 * abs(res["potential"]), (merged, res)
        one.calc_forces()
        slab.apply_stage(ranks)
        slab.finish_stage(ranks)
    one.close()
    for s in ranks:
        s.close()


def test_a_plan_that_lends_a_layer_is_refused_and_the_step_goes_on():
    xyz, age, v = slab_inputs(30000, 61)
    ranks = [ps.ParticleSystem(ps.default_config(rank=r, world=2, cuts=[0, 8, 16])) for r in range(2)]
    plans = [s.slab_plan() for s in ranks]
    assert plans[0].lentout_lo < plans[0].lentout_hi and plans[1].lentin_lo < plans[1].lentin_hi
    for s in ranks:
        s.fill_particles(xyz, age=age, fert_age=np.float32(1e6), vxyz=v)
    slab.to_pairs(ranks)
    for s in ranks:
        with pytest.raises(ps.PsamdError) as e:
            s.potential()
        assert e.value.status == ERR_UNSUPPORTED and "plan" in str(e.value)
    slab.apply_stage(ranks)
    slab.finish_stage(ranks)
    slab.step_local(ranks)
    for s in ranks:
        s.synchronize()
    assert sum(s.live_count() for s in ranks) > 0
    for s in ranks:
        s.close()


def test_a_slab_outside_its_window_is_refused():
    xyz, age, v = slab_inputs(20000, 61)
    ranks = [ps.ParticleSystem(ps.default_config(rank=r, world=2, cuts=[0, 7, 16])) for r in range(2)]
    for s in ranks:
        s.fill_particles(xyz, age=age, fert_age=np.float32(1e6), vxyz=v)

    def refused(s):
        with pytest.raises(ps.PsamdError) as e:
            s.potential()
        return e.value.status == ERR_STATE
    assert all(refused(s) for s in ranks)
    for s in ranks:
        s.slab_build()
    assert all(refused(s) for s in ranks)                        # the halos are not in yet
    slab.gather(ranks, slab.STATUS_OUT, slab.STATUS_IN)
    slab.deliver(ranks, "halo")
    for s in ranks:
        s.slab_pairs()
    assert all(s.potential()["listed"] > 0 for s in ranks)
    slab.apply_stage(ranks)
    assert all(refused(s) for s in ranks)
    slab.deliver(ranks, "xfer")
    for s in ranks:
        s.slab_finish()
        s.close()


# ---- state and arguments --------------------------------------------------------------------------------------------------

def test_state_and_arguments():
    n = 5000
    g = ps.ParticleSystem(ps.default_config())
    g.fill_particles(cloud(n, 71), age=np.float32(3.0), fert_age=np.float32(1e6), vxyz=cloud(n, 72, 20.0))
    dev = torch.device("cuda", 0)
    buf = torch.zeros(n + 8, dtype=torch.float32, device=dev)
    rec = torch.zeros(64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    good = dict(phi=buf.data_ptr(), capacity=n, result_dev=rec.data_ptr())

    def call(**kw):
        return g.lib.psamd_potential(g.h, C.byref(ps.Potential(**{**good, **kw})))
    assert call() == ERR_STATE                                   # no frame built
    with pytest.raises(ps.PsamdError) as e:
        g.download_potential()
    assert e.value.status == ERR_STATE
    g.init_iframe()
    assert call() == ERR_STATE
    g.build_grid()
    assert call() == 0
    for bad in (dict(flags=1), dict(reserved=1), dict(capacity=-1), dict(phi=buf.data_ptr() + 2), dict(phi=None),
                dict(result_dev=rec.data_ptr() + 4)):
        assert call(**bad) == ERR_INVALID_ARG, bad
    assert g.lib.psamd_potential(g.h, None) == ERR_INVALID_ARG and g.lib.psamd_potential(None, C.byref(ps.Potential())) == ERR_INVALID_ARG
    assert g.lib.psamd_potential_result_get(g.h, None) == ERR_INVALID_ARG
    assert g.lib.psamd_download_potential(g.h, None, 4, None) == ERR_INVALID_ARG
    assert g.lib.psamd_download_potential(g.h, None, -1, None) == ERR_INVALID_ARG
    assert call(phi=None, capacity=0, result_dev=None) == 0      # the context's own record alone
    assert call() == 0                                           # the refusals left the context usable
    e1, k = g.energy(), g.live_stats()["kinetic"]
    assert e1["kinetic"] == k and k > 0 and e1["total"] == e1["kinetic"] + e1["potential"] and e1["potential"] == g.potential_result()["potential"]
    g.calc_forces()
    assert call() == ERR_STATE                                   # the frame has ended
    g.synchronize()
    g.close()


# ---- a container that is no whole number of slot tiles (tests/test_gpu_export.py, ragged) ---------------------------------

def test_ragged_last_tile_pairs_with_the_export():
    g, rec = ragged(seed=33)
    open_frame(g)
    phi, ids, res = by_id(g)
    fr = Frame(g)
    live = g.live_count()
    assert len(ids) == live == res["listed"] and ids.max() >= 16384 and (np.diff(ids) > 0).all()
    check_against(fr, phi, res, fr.phi_cutoff(), "ragged last tile")
    d = g.download_potential()
    assert np.array_equal(bits(d["phi"]), bits(res["phi"]))
    g.close()


def test_ragged_capacity_cuts():
    g, rec = ragged(seed=34)
    open_frame(g)
    full = g.potential(phi=True)
    live = g.live_count()
    assert len(full["phi"]) == live == full["listed"]
    want = bits(full["phi"])
    dev = torch.device("cuda", 0)
    for cap in capacities(live):
        m = min(live, cap)
        out = torch.full((cap + 1,), SENTINEL, dtype=torch.int32, device=dev)
        result = torch.zeros(C.sizeof(ps.PotentialResult), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        spec = ps.Potential(phi=out.data_ptr() if cap > 0 else None, capacity=cap, result_dev=result.data_ptr())
        assert g.lib.psamd_potential(g.h, C.byref(spec)) == 0
        torch.cuda.ExternalStream(g.stream()).synchronize()
        a = out.cpu().numpy()
        assert np.array_equal(a[:m].view(np.uint32), want[:m]), "capacity %d: phi differs" % cap
        assert (a[m:] == SENTINEL).all(), "capacity %d: written past entry %d" % (cap, m)
        r = ps.PotentialResult.from_buffer_copy(result.cpu().numpy().tobytes()).to_dict()
        assert r == {k: full[k] for k in full if k != "phi"}, (cap, r)
        # the wrappers: the count they cut by is the live count
        short = g.potential(phi=True, capacity=cap)
        assert len(short["phi"]) == m and np.array_equal(bits(short["phi"]), want[:m]), cap
        if cap > 0:
            d = g.download_potential(capacity=cap)
            assert len(d["phi"]) == m and np.array_equal(bits(d["phi"]), want[:m]), cap
    g.close()
