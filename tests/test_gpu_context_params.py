"""The model of context creation's arithmetic (context_params_model.py) against a real context: what the device gets, not
only what csrc/context_params.hpp says.  Nine small configurations (8 to 16 cells per axis), one context each; checked are
the sizes of psamd_slab_buffers_get and which of its pointers are null, the sorted order's capacity, the owned slots and the
own cells of psamd_device_view_get, and psamd_get_slab_plan."""
import pytest

import particlesystem_amd as ps
from context_params_model import (ALL_PAIRS, ALLG_IN, ALLG_OUT, EXPLOSIONS, FAR_IN, FAR_MONOPOLE, FAR_OUT, FAR_PYRAMID, FAR_QUADRUPOLE,
                                  FAR_SLAB, FORCE_IN, FORCE_OUT, HALO_IN, HALO_OUT, STATUS_IN, STATUS_OUT, XFER2_IN, XFER2_OUT, XFER_IN,
                                  XFER_OUT, model_of, xfer_bytes)

pytestmark = pytest.mark.gpu
SMALL = dict(max_particles_num=4096)
G10 = dict(max_particles_num=4096, chunk_factor=2, chunk_dim=5)
CASES = {
    "world1": SMALL,
    "far_mono_world1": dict(SMALL, flags=FAR_MONOPOLE),
    "world2_lent_in": dict(SMALL, world=2, rank=1),
    "cuts4_rank1": dict(SMALL, world=4, rank=1, cuts=[0, 4, 7, 11, 16]),
    "single_layer_rank2": dict(collision_radius=0.0, chunk_factor=5, chunk_dim=3, max_particles_num=60000, cuts=[0, 2, 4, 6, 8, 10, 12, 15],
                               world=7, rank=2),
    "explosions4_rank0": dict(SMALL, flags=EXPLOSIONS, world=4, rank=0),
    "allpairs3_rank1": dict(G10, flags=ALL_PAIRS, world=3, rank=1),
    "far_quad_slab_rank0": dict(SMALL, flags=FAR_PYRAMID | FAR_QUADRUPOLE | FAR_SLAB, world=2, rank=0),
    "caps_rank1": dict(SMALL, world=3, rank=1, cuts=[0, 4, 7, 16], xfer_cap=64, xfer_cap_max=9000, halo_cap_cell=2),
}
PLAN_FIELDS = ("world", "rank", "grid_dim", None, None, "cut_lo", "cut_hi", "state_lo", "state_hi", None, None, "below_lo", "below_hi", "above_lo",
               "above_hi", "lentin_lo", "lentin_hi", "lentout_lo", "lentout_hi", "send_up_lo", "send_up_hi", "send_down_lo", "send_down_hi",
               "up_rank", "down_rank", None)     # the model's "plan" row; None: not in psamd_slab_plan


@pytest.mark.parametrize("name", list(CASES))
def test_a_context_has_what_the_model_derives(name):
    cfg = ps.default_config(**CASES[name])
    m = model_of(cfg)
    assert isinstance(m, dict), m
    msg = [m["msg.%d" % w] for w in range(20)]
    s = ps.ParticleSystem(cfg)
    try:
        b, v, p = s.slab_buffers(), s.device_view(), s.slab_plan()
    finally:
        s.close()
    ptr = {HALO_OUT: b.halo_out[0], HALO_OUT + 1: b.halo_out[1], HALO_IN: b.halo_in[0], HALO_IN + 1: b.halo_in[1], FORCE_OUT: b.force_out,
           FORCE_IN: b.force_in, XFER_OUT: b.xfer_out[0], XFER_OUT + 1: b.xfer_out[1], XFER_IN: b.xfer_in[0], XFER_IN + 1: b.xfer_in[1],
           STATUS_OUT: b.status_out, STATUS_IN: b.status_in, ALLG_OUT: b.allg_out, ALLG_IN: b.allg_in, XFER2_OUT: b.xfer2_out[0],
           XFER2_OUT + 1: b.xfer2_out[1], XFER2_IN: b.xfer2_in[0], XFER2_IN + 1: b.xfer2_in[1], FAR_OUT: b.far_out, FAR_IN: b.far_in}
    assert len(ptr) == 20
    for which, (nbytes, room) in enumerate(msg):
        assert bool(ptr[which]) == (room > 0), (name, which)
    assert [int(x) for x in b.halo_out_bytes] == [msg[HALO_OUT][0], msg[HALO_OUT + 1][0]]
    assert [int(x) for x in b.halo_in_bytes] == [msg[HALO_IN][0], msg[HALO_IN + 1][0]]
    assert (b.force_out_bytes, b.force_in_bytes) == (msg[FORCE_OUT][0], msg[FORCE_IN][0])
    assert b.xfer_bytes == msg[XFER_OUT][0] == msg[XFER_IN + 1][0] and b.xfer2_bytes == msg[XFER2_OUT][0] == msg[XFER2_IN + 1][0]
    assert b.xfer_bytes_max == (xfer_bytes(m["P.xfer_cap_max"][0] + 1) if cfg.world > 1 else 0)
    assert b.status_bytes == msg[STATUS_OUT][0] and b.status_bytes * cfg.world == msg[STATUS_IN][0]
    assert b.allg_bytes == msg[ALLG_OUT][0] and b.allg_bytes * cfg.world == msg[ALLG_IN][0]
    assert b.far_bytes == msg[FAR_OUT][0] and b.far_bytes * cfg.world == msg[FAR_IN][0]
    assert (v.sorted_cap, v.container_size, v.num_cells) == (m["P.sorted_cap"][0], m["P.slots_total"][0], m["P.n_own_cells"][0])
    assert [getattr(p, f) for f in PLAN_FIELDS if f] == [x for f, x in zip(PLAN_FIELDS, m["plan"]) if f]
    for f in ("slot_lo", "slot_hi", "rec_lo", "rec_hi"):
        assert list(getattr(p, f)) == m["plan." + f]


def test_the_cases_have_every_kind_of_message():
    """(no context needed) between them the cases above have each of the twenty messages, and each lacks some"""
    have = [[model_of(ps.default_config(**o))["msg.%d" % w][1] > 0 for w in range(20)] for o in CASES.values()]
    assert all(any(col) for col in zip(*have)) and not any(all(col) for col in zip(*have))
