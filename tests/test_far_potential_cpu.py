"""PSAMD_POTENTIAL_FAR / PSAMD_PROBE_FAR without a GPU (test_far_model_cpu.py has the two bits and
psamd_download_potential_far): the model's two forms agree (far_harness.py has the check, once for every method); and the METHOD -- the
stencil as a direct sum, the far set's monopoles behind it (far_model.py) -- against an fp64 direct sum over all
bodies: the far phi is nearer to it than the stencil-only phi, for the median particle, flat and as a pyramid.

Measured with the seeds below, 8192 bodies, 400 sampled per cloud, median / maximum relative deviation of phi from the
direct sum -- flat; pyramid; the stencil alone:
  8^3 uniform     1.1e-4 / 5.7e-4;  1.8e-4 / 1.1e-3;  0.87 / 0.94
  8^3 clustered   1.1e-4 / 7.2e-4;  2.7e-4 / 1.1e-3;  0.78 / 0.98
  10^3 uniform    8.6e-5 / 4.2e-4;  1.1e-3 / 5.2e-3;  0.91 / 0.96
  10^3 clustered  1.0e-4 / 5.1e-4;  4.4e-4 / 2.9e-3;  0.82 / 0.99
The model's fp32 association against its fp64 form: 1.3e-7 (flat), 1.9e-7 (pyramid)"""
import numpy as np
import pytest

import far_model as F
from far_harness import EPS2, W, phi_against_the_direct_sum, two_forms_of_the_model_agree


@pytest.mark.parametrize("G", [8, 10])
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_the_method_against_the_direct_sum(kind, G):
    dev = phi_against_the_direct_sum(kind, G)
    near = dev["stencil"]
    assert np.median(near) > 0.5                                     # (the far part is no small correction)
    for method in ("flat", "pyramid"):
        far = dev[method]
        print("%s cloud, 8192 bodies on %d^3 cells, %s: far phi median %.3g max %.3g; stencil alone median %.3g max %.3g"
              % (kind, G, method, np.median(far), far.max(), np.median(near), near.max()))
        assert np.median(far) < np.median(near)


@pytest.mark.parametrize("method", ["flat", "pyramid"])
def test_the_two_forms_of_the_model_agree(method):
    two_forms_of_the_model_agree(method)


def test_a_confined_cloud_has_no_far_body_and_one_level_is_the_flat_set():
    G = 8
    rng = np.random.default_rng(15)
    xyz = rng.uniform(-4.99, 4.99, (300, 3)).astype(np.float32)      # cells 3..4 on every axis
    w = np.full(300, W, np.float32)
    lists = F.lists_of(xyz, G)
    cell = F.cells_of(xyz, G)
    idx = np.arange(300)
    near = F.phi32(lists, xyz, w, G, EPS2, xyz, cell, idx, "flat", far=False)
    for method in ("flat", "pyramid"):
        assert np.array_equal(F.phi32(lists, xyz, w, G, EPS2, xyz, cell, idx, method), near)
    for c in range(64):
        assert F.far_set(c, 4, "pyramid") == F.far_set(c, 4, "flat")
