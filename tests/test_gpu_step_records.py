"""What the host shows of a step's scalar record, and when (csrc/step_ledger.hpp): `device_view().live` is read without
a sync -- the benchmark does so and takes it to lag a step.  The golden cloud of 4096 particles on the default grid,
explosions on, twelve single steps in two contexts: one that waits for every step's own record, one that runs ahead."""
import numpy as np
import pytest

import particlesystem_amd as ps
from util import g2_cloud

pytestmark = pytest.mark.gpu

STEPS = 12


def make(run_ahead):
    xyz = g2_cloud()
    rng = np.random.default_rng(12)
    age = rng.uniform(15 / 7, 7.5, len(xyz)).astype(np.float32)
    fert = rng.uniform(2.5, 9.0, len(xyz)).astype(np.float32)
    g = ps.ParticleSystem(ps.default_config(flags=ps.FLAG_EXPLOSIONS, seed=0xC0FFEE))
    g.fill_particles(xyz, age=age, fert_age=fert)
    g.set_run_ahead(run_ahead)
    return g


def test_live_count_of_the_view_lags_by_the_run_ahead_and_no_more():
    now, ahead = make(0), make(1)
    fresh = int(ahead.device_view().live)
    # no run-ahead: after every step, the particles that step's build_grid found (counted from the slots before the step)
    at_build = []
    for s in range(STEPS):
        at_build.append(now.live_count())
        now.step(1)
        assert int(now.device_view().live) == at_build[s], s + 1
    assert len(set(at_build)) > 1                   # (the population moves: a stale figure would show)
    # run-ahead 1, nothing waits in between: step s - 1's figure, or step s's where its record has arrived already
    for s in range(STEPS):
        ahead.step(1)
        assert int(ahead.device_view().live) in ((at_build[s - 1] if s else fresh), at_build[s]), s + 1
    now.synchronize(); ahead.synchronize()
    assert int(now.device_view().live) == int(ahead.device_view().live) == at_build[-1]
    cn, ca = now.counters, ahead.counters
    assert cn["particles_processed"] == ca["particles_processed"] == sum(at_build)
    assert cn["max_ops_one_queue"] == ca["max_ops_one_queue"]
    now.close(); ahead.close()
