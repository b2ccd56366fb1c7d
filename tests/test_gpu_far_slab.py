"""Far-field gravity on slabs (PSAMD_FLAG_FAR_SLAB): every rank all-gathers the fp64 sums of its own cells, and the union of
the ranks is one context's state byte for byte -- the moments on every rank, the force records, whole steps.  Every check is a
byte comparison against a one-context run WITHOUT the flag (the code path the flag does not touch), so no tolerance is involved.
Small grids (far_harness.GRID, 16 384-slot containers), a few thousand particles, step_local and merge_owned."""
import functools
import os
import subprocess

import numpy as np
import pytest

import particlesystem_amd as ps
from far_harness import GRID, INVALID_ARG, UNSUPPORTED, box_cloud, status_of_create
from particlesystem_amd import slab
from particlesystem_amd.slab import apply_stage, finish_stage, merge_owned, step_local, to_pairs
from util import assert_same_particles

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = {"flat": ps.FLAG_FAR_MONOPOLE, "pyramid": ps.FLAG_FAR_PYRAMID, "quadrupole": ps.FLAG_FAR_PYRAMID | ps.FLAG_FAR_QUADRUPOLE}
UNEVEN_CUTS = (0, 3, 7, 11, 16)
# (grid, world, cuts): default cuts at 8^3 on two ranks (a lent layer); 10^3 on three (chunk_dim 5: an odd level with a ragged parent,
# two lent layers); the uneven cuts at 16^3 on four; 16^3 on eight (every rank but the last lends a layer)
SHAPES = [(8, 2, None), (10, 3, None), (16, 4, UNEVEN_CUTS), (16, 8, None)]
N = {8: 3000, 10: 4000, 16: 6000}
STEPS = 5


def the_cloud(G):
    """spread over the whole box, kids among the adults, velocities that carry particles over cell faces and slab cuts within
    a few steps; the default collision radius makes some of them collide"""
    n = N[G]
    rng = np.random.default_rng(70 + G)
    age = rng.uniform(15 / 7, 7.5, n).astype(np.float32)
    age[::23] = 0.5
    return dict(xyz=box_cloud(n, 70 + G, G), age=age, fert_age=(1e6 + np.arange(n)).astype(np.float32),
                vxyz=rng.uniform(-8, 8, (n, 3)).astype(np.float32))


def one_context(G, flags, **cfg):
    g = ps.ParticleSystem(ps.default_config(flags=flags, **GRID[G], **cfg))
    assert g.sizes.grid_dim == G
    g.fill_particles(**the_cloud(G))
    return g


def slabs(G, world, cuts, flags, **cfg):
    over = dict(GRID[G], **cfg)
    if cuts:
        over["cuts"] = cuts
    ranks = [ps.ParticleSystem(ps.default_config(flags=flags | ps.FLAG_FAR_SLAB, rank=r, world=world, **over)) for r in range(world)]
    for g in ranks:
        g.fill_particles(**the_cloud(G))
    return ranks, [g.slab_plan() for g in ranks]


def close(*systems):
    for g in systems:
        g.close()


@functools.lru_cache(maxsize=None)
def one_context_steps(G, flags, steps=STEPS):
    """the one-context run, computed once per (grid, force model): (the particles after every step, the counters)"""
    g = one_context(G, flags)
    after = []
    for _ in range(steps):
        g.step(1)
        after.append(g.download_particles())
    c = dict(g.counters)
    g.close()
    return after, c


def sent_to_another_rank(ranks):
    """records in the transfer messages of the step that just ended: particles that changed owner"""
    return sum(int(g.msg_download(slab.XFER_OUT + k)[0]) for g in ranks for k in (0, 1))


# ---- 1. the union equals one context, every step ----------------------------------------------------------------------------------

@pytest.mark.parametrize("G,world,cuts", SHAPES)
@pytest.mark.parametrize("method", list(METHODS))
def test_union_of_far_slabs_is_one_context_every_step(method, G, world, cuts):
    flags = METHODS[method]
    want, counters = one_context_steps(G, flags)
    ranks, plans = slabs(G, world, cuts, flags)
    moved = 0
    for step in range(STEPS):
        step_local(ranks)
        moved += sent_to_another_rank(ranks)
        union = merge_owned([g.download_particles() for g in ranks], plans)
        assert_same_particles(union, want[step], "%s, %d^3 on %d slabs, step %d" % (method, G, world, step + 1))
    print("%s %d^3 x %d: %d relocations, %d collision deaths, %d owner changes" % (method, G, world, counters["relocations"],
                                                                                 counters["deaths_collision"], moved))
    assert counters["relocations"] > 0 and counters["deaths_collision"] > 0 and counters["integrated"] > 0
    assert counters["cell_overflow_kills"] == 0
    assert moved > 0, "no particle changed owner: the inputs do not exercise the transfer"
    # the far field really is in the sums: the cutoff run of the same cloud differs after one step
    cut, _ = one_context_steps(G, 0, 1)
    assert cut[0].tobytes() != want[0].tobytes()
    close(*ranks)


# ---- 2. the moments on every rank ---------------------------------------------------------------------------------------------------

def moments_of(g):
    levels = range(len(ps.far_levels(g.cfg)))
    out = {}
    if g.cfg.flags & ps.FLAG_FAR_PYRAMID:
        out["mom"] = [g.download_level_moments(l) for l in levels]
    else:
        out["mom"] = [g.download_cell_moments()]
    if g.cfg.flags & ps.FLAG_FAR_QUADRUPOLE:
        out["cen"] = [g.download_level_quadrupoles(l) for l in levels]
    return out


@pytest.mark.parametrize("G,world,cuts,sign", [(8, 2, None, 1.0), (10, 3, None, -1.0), (16, 4, UNEVEN_CUTS, 1.0)])
@pytest.mark.parametrize("method", list(METHODS))
def test_every_rank_holds_the_moments_of_one_context(method, G, world, cuts, sign):
    flags = METHODS[method]
    one = one_context(G, flags, force_sign=sign)
    one.init_iframe(); one.build_grid(); one.calc_forces_pairs()
    want = moments_of(one)
    ranks, _ = slabs(G, world, cuts, flags, force_sign=sign)
    to_pairs(ranks)
    for r, g in enumerate(ranks):
        got = moments_of(g)
        assert sorted(got) == sorted(want)
        for kind in want:
            assert len(want[kind]) == len(got[kind])
            for l, (a, b) in enumerate(zip(got[kind], want[kind])):
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: rank %d, level %d, %s" % (method, r, l, kind)
    assert np.count_nonzero(want["mom"][0][:, 3]) > G ** 3 // 2        # (the cells hold mass: equal zeros would prove nothing)
    apply_stage(ranks); finish_stage(ranks)                           # the frame ends as frames do
    for g in ranks:
        g.synchronize()
    close(one, *ranks)


# ---- 3. the force records -----------------------------------------------------------------------------------------------------------

def records_by_slot(g, layers=None):
    """{slot id: 16 bytes of record} of the cells of the rank's own block (of those in the given global layers)"""
    rows = g.download_cellgrid()
    G = g.sizes.grid_dim
    counts = rows[:, 0]
    cells = np.nonzero(counts)[0]
    order = np.concatenate([rows[c, 1:1 + rows[c, 0]] for c in cells])
    layer = np.concatenate([np.full(rows[c, 0], c // (G * G)) for c in cells])
    f = g.download_force4(0, len(order))
    f = np.ascontiguousarray(f).view(np.uint32).reshape(len(order), 4)
    keep = np.ones(len(order), bool) if layers is None else (layer >= layers[0]) & (layer < layers[1])
    return dict(zip(order[keep].tolist(), f[keep]))


@pytest.mark.parametrize("G,world,cuts", [(16, 4, UNEVEN_CUTS), (16, 4, None), (16, 8, None)])
@pytest.mark.parametrize("method", list(METHODS))
def test_force_records_of_every_computed_cell_are_one_contexts(method, G, world, cuts):
    """the cells a rank computes and owns: their records after slab_pairs; the cells it computes for the rank below (lent-in
    layers): where they land, in the owner's particles after slab_apply (a particle that moves keeps its record as its stored
    acceleration).  The cuts (0, 3, 7, 11, 16) fall on group boundaries of this plan, so nothing is lent there; the default cuts
    lend a layer at every cut, in a world of four and of eight."""
    flags = METHODS[method]
    one = one_context(G, flags)
    one.init_iframe(); one.build_grid(); one.calc_forces_pairs()
    want = records_by_slot(one)
    assert one.counters["cell_overflow_kills"] == 0
    ranks, plans = slabs(G, world, cuts, flags)
    to_pairs(ranks)
    own = lent = 0
    for g, p in zip(ranks, plans):
        got = records_by_slot(g, (max(p.cut_lo, p.state_lo), min(p.cut_hi, p.state_hi)))
        for s, rec in got.items():
            assert rec.tobytes() == want[s].tobytes(), "%s: rank %d, slot %d" % (method, p.rank, s)
        own += len(got)
    apply_stage(ranks)
    for g, p in zip(ranks, plans):
        if p.lentout_lo == p.lentout_hi:
            continue
        for s, rec in records_by_slot(g, (p.lentout_lo, p.lentout_hi)).items():
            if want[s][3] == 0:                                   # (flag 0: the particle moves and keeps its record)
                assert rec[:3].tobytes() == want[s][:3].tobytes(), "%s: lent layer of rank %d, slot %d" % (method, p.rank, s)
                lent += 1
    finish_stage(ranks)
    lends = any(p.lentout_lo != p.lentout_hi for p in plans)
    assert lends == (cuts is None)                                # (what the plan says of these cuts, see above)
    assert own > N[G] // 2 and lent > (100 if lends else -1), (own, lent)
    assert len({tuple(v[:3]) for v in want.values()}) > N[G] // 2
    close(one, *ranks)


# ---- 4. modes -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["fast_math", "explosions_graphs", "explosions_no_graphs", "overlap_interior"])
def test_far_slabs_in_every_mode(mode):
    G, world = 8, 2
    flags = ps.FLAG_FAR_PYRAMID | {"fast_math": ps.FLAG_FAST_MATH, "overlap_interior": 0}.get(mode, ps.FLAG_EXPLOSIONS)
    graphs = mode != "explosions_no_graphs"
    cloud = the_cloud(G)
    if mode.startswith("explosions"):
        cloud["fert_age"] = (cloud["age"] + 0.05 * (1 + np.arange(len(cloud["age"])) % 3)).astype(np.float32)      # births within the three steps
    one = ps.ParticleSystem(ps.default_config(flags=flags, **GRID[G]))
    ranks = [ps.ParticleSystem(ps.default_config(flags=flags | ps.FLAG_FAR_SLAB, rank=r, world=world, **GRID[G])) for r in range(world)]
    for g in [one] + ranks:
        g.fill_particles(**cloud)
        g.set_graphs(graphs)
    plans = [g.slab_plan() for g in ranks]
    for step in range(3):
        one.step(1)
        step_local(ranks, overlap_interior=mode == "overlap_interior")
        union = merge_owned([g.download_particles() for g in ranks], plans)
        assert_same_particles(union, one.download_particles(), "%s, step %d" % (mode, step + 1))
    if mode.startswith("explosions"):
        assert one.counters["births"] > 0
    close(one, *ranks)


# ---- 5. the flag's rules --------------------------------------------------------------------------------------------------------------

def test_flag_rules():
    for flags in METHODS.values():
        assert status_of_create(flags=flags, rank=0, world=2, **GRID[8]) == UNSUPPORTED          # (as on the parent)
    for world in (1, 2):
        assert status_of_create(flags=ps.FLAG_FAR_SLAB, rank=0, world=world, **GRID[8]) == INVALID_ARG
        assert status_of_create(flags=ps.FLAG_FAR_SLAB | ps.FLAG_ALL_PAIRS, rank=0, world=world, **GRID[8]) == INVALID_ARG
    assert status_of_create(flags=ps.FLAG_FAR_SLAB | ps.FLAG_ALL_PAIRS | ps.FLAG_FAR_PYRAMID, rank=0, world=2, **GRID[8]) == INVALID_ARG
    assert status_of_create(flags=ps.FLAG_FAR_SLAB | ps.FLAG_FAR_QUADRUPOLE, **GRID[8]) == INVALID_ARG


@pytest.mark.parametrize("method", list(METHODS))
def test_the_flag_on_one_context_changes_nothing(method):
    G = 8
    want, _ = one_context_steps(G, METHODS[method], 3)
    g = one_context(G, METHODS[method] | ps.FLAG_FAR_SLAB)
    assert g.msg_bytes(ps.MSG_ALLG_OUT) == 0 and g.msg_bytes(ps.MSG_ALLG_IN) == 0
    for step in range(3):
        g.step(1)
        assert_same_particles(g.download_particles(), want[step], "%s with the flag, world 1, step %d" % (method, step + 1))
    g.close()


# ---- 6. the message's shape -----------------------------------------------------------------------------------------------------------

def test_message_shape():
    G, world = 16, 4
    size = {}
    for method, flags in METHODS.items():
        ranks = [ps.ParticleSystem(ps.default_config(flags=flags | ps.FLAG_FAR_SLAB, rank=r, world=world, cuts=UNEVEN_CUTS, **GRID[G]))
                 for r in range(world)]
        plans = [g.slab_plan() for g in ranks]
        out = [g.msg_bytes(ps.MSG_ALLG_OUT) for g in ranks]
        assert out[0] > 0 and len(set(out)) == 1
        assert all(g.msg_bytes(ps.MSG_ALLG_IN) == world * out[0] for g in ranks)
        layers = [p.state_hi - p.state_lo for p in plans]
        assert len(set(layers)) > 1                                # the cuts are uneven: the blocks are sized for the largest
        allg_cells, planes = max(layers) * G * G, 10 if method == "quadrupole" else 4
        assert out[0] == 64 + planes * allg_cells * 8             # the header, then the planes of doubles: 8-byte aligned, nothing to round
        size[method] = out[0]
        # ... and the header a rank writes says what the plan says of it
        for g in ranks:
            g.fill_particles(**the_cloud(G))
            g.slab_build()
        for g, p in zip(ranks, plans):
            hdr = g.msg_download(ps.MSG_ALLG_OUT)[:4]
            assert hdr.tolist() == [(p.state_hi - p.state_lo) * G * G, planes, 0, p.state_lo * G * G]
        close(*ranks)
    assert size["quadrupole"] > size["pyramid"] == size["flat"]


# ---- 7. a block that did not arrive is loud -------------------------------------------------------------------------------------------

def test_a_block_left_out_is_loud():
    """One rank's block zeroed in one rank's allg_in: a bad header (it names no cells), which the scatter checks before it
    touches anything; the step fails collectively, as a far outbox left out does (test_gpu_slab.py)."""
    G, world = 8, 2
    ranks, _ = slabs(G, world, None, ps.FLAG_FAR_PYRAMID)
    step_local(ranks)                                              # with every block: fine
    for g in ranks:
        g.synchronize()

    def spoil():
        words = ranks[1].msg_download(ps.MSG_ALLG_IN)
        block = len(words) // world
        words[:block] = 0                                          # rank 0's block never arrived on rank 1
        ranks[1].msg_upload(ps.MSG_ALLG_IN, words)

    with pytest.raises(ps.PsamdError, match="does not match"):
        to_pairs(ranks, before_pairs=spoil)
        apply_stage(ranks); finish_stage(ranks)
        for g in ranks:
            g.synchronize()
        step_local(ranks)                                          # (raised in the pair stage, reported collectively with the next step's status)
        for g in ranks:
            g.synchronize()
    close(*ranks)


# ---- 8. potential and probe are refused, the step goes on --------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["pyramid", "quadrupole"])
def test_services_are_refused_and_the_step_completes(method):
    import torch
    G, world = 8, 2
    flags = METHODS[method]
    want, _ = one_context_steps(G, flags)
    ranks, plans = slabs(G, world, None, flags)
    quad = method == "quadrupole"
    to_pairs(ranks)
    for g in ranks:
        with pytest.raises(ps.PsamdError) as e:
            g.potential(far=True, quadrupole=quad)
        assert e.value.status == UNSUPPORTED
        with pytest.raises(ps.PsamdError) as e:
            g.download_potential(far=True, quadrupole=quad)
        assert e.value.status == UNSUPPORTED
        pos4 = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
        with pytest.raises(ps.PsamdError) as e:
            g.probe(pos4, acc=True, phi=False, far=True, quadrupole=quad)
        assert e.value.status == UNSUPPORTED
    apply_stage(ranks); finish_stage(ranks)
    union = merge_owned([g.download_particles() for g in ranks], plans)
    assert_same_particles(union, want[0], "%s after the refusals" % method)
    step_local(ranks)                                              # the contexts stay usable
    union = merge_owned([g.download_particles() for g in ranks], plans)
    assert_same_particles(union, want[1], "%s, the step after" % method)
    close(*ranks)


# ---- 9. the C++ ring host -------------------------------------------------------------------------------------------------------------

@pytest.mark.timeout(300)
@pytest.mark.parametrize("far", ["pyramid", "quadrupole"])
def test_ring_host_loopback_with_the_far_field(far):
    exe = ps._build.build_ring()
    p = subprocess.run(["timeout", "-k", "10", "240", exe, "--loopback", "--world", "3", "--far", far, "--n", "20000", "--iters", "4"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=280)
    print(p.stdout[-1500:])
    assert p.returncode == 0, p.stdout[-3000:]
    assert "ring-rccl ok: 0 of" in p.stdout
