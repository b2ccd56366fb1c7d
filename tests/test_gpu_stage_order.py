"""The order of the stage calls on the device (csrc/frame_stage.hpp).

World 1: a call of one family inside a frame of the other is refused (PSAMD_ERR_STATE), enqueues nothing and leaves the
stage where it was -- the frame is finished by its own family and the steps that follow equal the CPU oracle byte for byte.
World 2: the orders the flag machine refused are refused as before (each expectation comes from its transcription in
test_frame_stage_cpu.py), a second slab_pairs_interior stays a silent no-op, potential and probe are served between
slab_pairs and slab_apply only, and the steps that follow equal the oracle's slab merge."""
import numpy as np
import pytest

import oracle_py as O
import particlesystem_amd as ps
from particlesystem_amd import slab
from particlesystem_amd.slab import step_local
from test_frame_stage_cpu import old_call
from service_harness import ERR_STATE, compare_world, make_world
from util import assert_same_particles, cloud, oracle_cfg_from

pytestmark = pytest.mark.gpu

GRID = {"chunk_factor": 2, "chunk_dim": 4, "max_particles_num": 4000}       # 8^3 cells
N = 2000
AGE, FERT = np.float32(3.0), np.float32(1e6)


def inputs():
    return cloud(N, 91, 20.0)


@pytest.fixture(scope="module")
def oracle_steps():
    """particles, QUEUE_INFO and queue of the one-context oracle after steps 1, 2 and 3 (computed once, left unchanged)"""
    o = O.System(oracle_cfg_from(ps.default_config(**GRID)))
    o.fill(inputs(), age=AGE, fert_age=FERT)
    out = []
    for _ in range(3):
        o.step(1)
        out.append((o.particles.tobytes(), o.queue_info.tobytes(), o.queue.copy()))     # (bytes: a copy of a record array leaves its pad bytes undefined)
    o.close()
    return out


def same_as(g, want, what):
    p, qi, q = want
    got = g.download_particles()
    assert_same_particles(got, np.frombuffer(p, got.dtype), what)
    got_qi, got_q = g.download_queues()
    assert got_qi.tobytes() == qi, what + ": QUEUE_INFO differs"
    assert np.array_equal(got_q, q), what + ": queue array differs"


# (the calls before, the call that is refused, the frame's own family finishing it)
MIXED = [
    (("slab_build",), "init_iframe", ("slab_pairs", "slab_apply", "slab_finish")),
    (("slab_build", "slab_pairs"), "calc_forces_apply", ("slab_apply", "slab_finish")),
    (("slab_build",), "calc_forces_pairs", ("slab_pairs", "slab_apply", "slab_finish")),
    (("slab_build", "slab_pairs", "slab_apply"), "calc_forces_apply", ("slab_finish",)),
    (("slab_build",), "step", ("slab_pairs", "slab_apply", "slab_finish")),
    (("slab_build", "slab_pairs"), "calc_forces_pairs", ("slab_apply", "slab_finish")),
    (("slab_build", "slab_pairs", "slab_apply"), "init_iframe", ("slab_finish",)),
    (("init_iframe", "build_grid"), "slab_build", ("calc_forces",)),
    (("init_iframe", "build_grid", "calc_forces_pairs"), "slab_build", ("calc_forces_apply",)),
]


@pytest.mark.parametrize("before, offender, after", MIXED, ids=["%s;%s" % (";".join(b), k) for b, k, _ in MIXED])
def test_world_one_refuses_a_call_of_the_other_family(oracle_steps, before, offender, after):
    g = ps.ParticleSystem(ps.default_config(**GRID))
    g.fill_particles(inputs(), age=AGE, fert_age=FERT)
    g.set_graphs(True)                                  # (so that graph_stats counts every stage sequence submitted)
    for call in before:
        getattr(g, call)()
    stats, steps = g.graph_stats(), g.counters["steps"]
    with pytest.raises(ps.PsamdError) as e:
        getattr(g, offender)()
    assert e.value.status == ERR_STATE
    assert "slab_build" in str(e.value) and "init_iframe" in str(e.value)           # the text names both families
    assert g.graph_stats() == stats and g.counters["steps"] == steps
    for call in after:
        getattr(g, call)()
    assert g.counters["steps"] == steps + 1
    same_as(g, oracle_steps[0], "the frame the refused call was in")
    g.step(1)
    same_as(g, oracle_steps[1], "step(1) after it")
    step_local([g])
    same_as(g, oracle_steps[2], "step_local after it")
    g.close()


def test_world_two_orders_and_the_field_window():
    import torch
    ranks, o = make_world(2, inputs(), AGE, FERT, cuts=[0, 3, 8], **GRID)
    for s in ranks:
        s.set_graphs(True)
    flags = [(False, False, False, 0, False) for _ in ranks]        # the flag machine's state, rank by rank
    pts = torch.from_numpy(np.concatenate([cloud(64, 92, 20.0), np.zeros((64, 1), np.float32)], 1)).cuda()

    def call(name):
        """every rank makes the call; refused or not as the flag machine had it"""
        for r, s in enumerate(ranks):
            then = old_call(flags[r], name, 2, True)
            if then is None:
                before = (s.graph_stats(), s.counters["steps"])
                with pytest.raises(ps.PsamdError) as e:
                    getattr(s, name)()
                assert e.value.status == ERR_STATE and (s.graph_stats(), s.counters["steps"]) == before, (name, r)
            else:
                getattr(s, name)()
                flags[r] = then
        return then is not None

    def field(served):
        for s in ranks:
            if served:
                assert s.potential()["listed"] > 0
                r = s.probe(pts)
                assert r["done"] == 64 and r["served"] > 0
            else:
                for ask in (s.potential, lambda: s.probe(pts)):
                    with pytest.raises(ps.PsamdError) as e:
                        ask()
                    assert e.value.status == ERR_STATE

    field(False)
    assert not call("slab_pairs")                       # before slab_build
    assert not call("slab_pairs_interior") and not call("slab_apply") and not call("slab_finish")
    assert call("slab_build")
    assert not call("slab_apply")                       # before slab_pairs
    assert not call("slab_finish")
    field(False)                                        # the halos are not in yet
    slab.gather(ranks, slab.STATUS_OUT, slab.STATUS_IN)
    assert call("slab_pairs_interior")
    stats = [s.graph_stats() for s in ranks]
    assert call("slab_pairs_interior")                  # a second one: accepted, and nothing runs
    assert [s.graph_stats() for s in ranks] == stats
    slab.deliver(ranks, "halo")
    assert call("slab_pairs")
    assert not call("slab_pairs_interior")              # after slab_pairs
    assert not call("slab_pairs") and not call("slab_finish")       # ... twice; before slab_apply
    field(True)
    slab.deliver(ranks, "force")
    assert call("slab_apply")
    field(False)
    assert not call("slab_apply") and not call("slab_pairs")
    slab.deliver(ranks, "xfer")
    assert call("slab_finish")
    assert not call("slab_finish")
    field(False)
    o.step(1)
    compare_world(ranks, o, "the frame stepped among the refusals")
    for step in range(2):
        step_local(ranks); o.step(1)
        compare_world(ranks, o, "step_local %d after it" % (step + 1))
    for s in ranks:
        s.close()
