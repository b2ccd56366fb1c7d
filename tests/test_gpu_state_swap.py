"""Replacing or growing the particles while a step is in flight: psamd_upload_particles, psamd_fill_particles and
psamd_snapshot_restore called behind a step whose record the host has not read, then three steps in one call.

Two launches of a step are sized from the host's bound of the live count and must still reach every particle: the far walks
(k_allp_far, k_far_walk) and their combine (k_allpairs_combine; far_dense_bound, allpairs.hip).  They go by the device's own
count in rounds, so a launch that is too small costs time and no particle.  Since the ledger keeps the bound above the
particles alive through these calls (tests/test_step_ledger_cpu.py holds it to a simulated population) the rounds are a
second line; on the library before that -- where the record of the step enqueued before the call, read afterwards, put
the bound at the small population's -- the second step after the call went through the rounds in the twelve run-ahead
cases (a launch for the 40 or 2560 particles of that record: 2 and about 42 dense tasks of 64 where 313 and 320 were due): all
15 cases passed there, and with the three loops cut to one round those twelve failed (CHANGELOG.md).

What is compared: a context stepped once WITHOUT a synchronize, given about 20 000 particles by one of the three calls and
stepped three times in one call, against a fresh context that was given the same particles and queues with nothing in
flight and stepped three times -- particles, QUEUE_INFO records and queues byte for byte; and after a synchronize
device_view().live and live_count() against the live records of the download.  In all-pairs mode and with each far-field
method; a plain cutoff context against the CPU oracle is the control (no launch of its step goes by the bound)."""
import numpy as np
import pytest

import particlesystem_amd as ps
from util import O, assert_same_particles, cloud, oracle_cfg_from

pytestmark = pytest.mark.gpu

FLAGS = {"all_pairs": ps.FLAG_ALL_PAIRS, "monopole": ps.FLAG_FAR_MONOPOLE, "pyramid": ps.FLAG_FAR_PYRAMID,
         "quadrupole": ps.FLAG_FAR_PYRAMID | ps.FLAG_FAR_QUADRUPOLE}
ADULT, NEVER = np.float32(2.0), np.float32(1e6)        # past kid_age = 1.5, far from particle_life = 15; no births
# the default 16^3 cells of 5.0 with room for 34 particles each (139 264 slots: a download is 10 MB, not 150).  The routes
# that keep every particle alive run with a collision radius no pair of a random cloud is within, so that the live count at
# the last build_grid (device_view().live) is the count of the download.
SMALL_BOX = dict(max_particles_num=65536, seed=3)
NO_KILLS = dict(collision_radius=1e-3, **SMALL_BOX)
N_BIG = 20000


def make(flags, run_ahead=1, graphs=False, **cfg):
    g = ps.ParticleSystem(ps.default_config(flags=flags, **cfg))
    assert g.sizes.grid_dim == 16
    g.set_graphs(graphs)
    g.set_run_ahead(run_ahead)
    return g


def small(flags, **kw):
    """40 adults, one step enqueued and nothing waited for: its record is unread when the particles change"""
    g = make(flags, **kw)
    g.fill_particles(cloud(40, 77), age=ADULT, fert_age=NEVER)
    assert g.lib.psamd_step(g.h, 1) == 0
    return g


def big():
    """20 000 adults, a cell's width inside the box: nobody leaves it in four steps"""
    rng = np.random.default_rng(5)
    return dict(xyz=cloud(N_BIG, 5, half=35.0), vxyz=rng.uniform(-5, 5, (N_BIG, 3)).astype(np.float32), age=ADULT, fert_age=NEVER)


def fill_big(g):
    g.fill_particles(**big())


def fresh_with(state, flags, **cfg):
    """the reference: a context nothing is in flight on, given the particles and the queues"""
    p, qi, q = state
    c = make(flags, **cfg)
    c.upload_particles(p)
    c.upload_queues(qi, q)
    return c


def state_of(g):
    qi, q = g.download_queues()
    return g.download_particles(), qi, q


def same_state(a, b, what):
    (pa, qia, qa), (pb, qib, qb) = state_of(a), state_of(b)
    assert_same_particles(pa, pb, what + ": particles")
    assert qia.tobytes() == qib.tobytes(), what + ": QUEUE_INFO records differ"
    assert np.array_equal(qa, qb), what + ": queues differ"


def live_records(g):
    p = g.download_particles()
    return int(((p["cell"] >= 0) & (p["cell"] < g.sizes.num_cells)).sum())


def three_steps_and_compare(a, ref, what, expect_live):
    assert a.lib.psamd_step(a.h, 3) == 0              # one call: the second step is the one sized behind the stale record
    ref.step(3)
    same_state(a, ref, what)
    a.synchronize()
    n = live_records(a)
    assert n == expect_live, (what, n)
    assert a.device_view().live == n, (what, a.device_view().live, n)
    assert a.live_count() == n, what
    for g in (a, ref):
        g.close()


def by_upload(flags, run_ahead=1, graphs=False):
    src = make(flags, **NO_KILLS)                     # the state of another context, one step old
    fill_big(src)
    src.step(1)
    state = state_of(src)
    src.close()
    a = small(flags, run_ahead=run_ahead, graphs=graphs, **NO_KILLS)
    a.upload_particles(state[0])
    a.upload_queues(state[1], state[2])
    ref = fresh_with(state, flags, graphs=graphs, **NO_KILLS)
    three_steps_and_compare(a, ref, "upload behind a step", N_BIG)


def by_fill(flags):
    b = small(flags, **NO_KILLS)                      # the same calls with a wait in between, for the state after the fill
    b.synchronize()
    fill_big(b)
    state = state_of(b)
    b.close()
    a = small(flags, **NO_KILLS)
    fill_big(a)
    three_steps_and_compare(a, fresh_with(state, flags, **NO_KILLS), "fill behind a step", N_BIG + 40)


def clumps():
    """2560 clumps of 8 adults, a clump to a cell, the default collision radius of 0.4: the corners of a cube of edge 1.5
    about the cell's centre, each flying at the centre so as to be there after three steps (3 v dt = the offset; the
    masses are small enough for the flight to be straight).  The cube's edge at the builds of steps 1 to 4 is 1.5, 1.0,
    0.5 and 0: three steps kill nobody, the fourth all but one of every clump, and the survivors, a cell apart, meet
    nobody afterwards.  (A particle that collides takes no force in that step, so the steps that must be stepped
    through the rounds are the ones before the kill.)"""
    i = np.arange(16)
    i1, i2, i3 = (v.ravel() for v in np.meshgrid(i, i, i, indexing="ij"))
    keep = (i1 + i2 + i3) % 8 < 5
    centre = np.stack([i1, i2, i3], 1)[keep] * 5.0 - 37.5
    corner = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * 0.75
    xyz = (centre[:, None, :] + corner[None, :, :]).reshape(-1, 3).astype(np.float32)
    vxyz = np.tile(-corner / (3 * 0.05), (len(centre), 1)).astype(np.float32)
    return dict(xyz=xyz, vxyz=vxyz, age=ADULT, fert_age=NEVER, w=np.float32(0.01)), len(centre)


def by_restore(flags):
    c, n_clumps = clumps()
    n = 8 * n_clumps
    a = make(flags, **SMALL_BOX)
    a.fill_particles(**c)
    state = state_of(a)
    a.snapshot_save()
    a.step(3)
    assert a.live_count() == n                        # (the three steps after the restore repeat these)
    a.step(1)
    assert a.live_count() == n_clumps and n_clumps < n // 4
    assert a.lib.psamd_step(a.h, 1) == 0              # in flight: its record says n_clumps particles
    a.snapshot_restore()
    three_steps_and_compare(a, fresh_with(state, flags, **SMALL_BOX), "restore behind a step", n)


@pytest.mark.parametrize("flags", sorted(FLAGS))
def test_upload_behind_a_step(flags):
    by_upload(FLAGS[flags])


@pytest.mark.parametrize("flags", sorted(FLAGS))
def test_fill_behind_a_step(flags):
    by_fill(FLAGS[flags])


@pytest.mark.parametrize("flags", sorted(FLAGS))
def test_restore_behind_a_step(flags):
    by_restore(FLAGS[flags])


def test_all_pairs_upload_without_run_ahead():
    """every step reads its own record: nothing is stale, the calls stay right"""
    by_upload(ps.FLAG_ALL_PAIRS, run_ahead=0)


def test_all_pairs_upload_under_graphs():
    """the bound is rounded up to 64 Ki there, which covers these particles whatever the ledger holds: the calls stay right"""
    by_upload(ps.FLAG_ALL_PAIRS, graphs=True)


def test_cutoff_fill_behind_a_step_against_the_oracle():
    """the control: no launch of a cutoff step goes by the bound"""
    g = small(0, **NO_KILLS)
    o = O.System(oracle_cfg_from(g.cfg))
    o.fill(cloud(40, 77), age=ADULT, fert_age=NEVER)
    o.step(1)
    fill_big(g)
    b = big()
    ids = o.fill(b["xyz"], age=ADULT, fert_age=NEVER)
    p = o.particles
    p["vx"][ids], p["vy"][ids], p["vz"][ids] = b["vxyz"].T
    assert g.lib.psamd_step(g.h, 3) == 0
    o.step(3)
    assert_same_particles(g.download_particles(), o.particles, "cutoff, fill behind a step, against the oracle")
    qi, q = g.download_queues()
    assert qi.tobytes() == o.queue_info.tobytes() and np.array_equal(q, o.queue)
    g.synchronize()
    n = live_records(g)
    assert n == N_BIG + 40 and g.device_view().live == n and g.live_count() == n
    g.close()
    o.close()
