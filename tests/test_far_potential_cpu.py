"""PSAMD_POTENTIAL_FAR / PSAMD_PROBE_FAR without a GPU (test_far_model_cpu.py has the two bits and
psamd_download_potential_far): the model's two forms agree; and the METHOD -- the
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
from far_harness import EPS2, W, cloud_frame


@pytest.mark.parametrize("G", [8, 10])
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_the_method_against_the_direct_sum(kind, G):
    xyz, w, lists = cloud_frame(kind, G)
    pick = np.random.default_rng(13).choice(len(xyz), 400, replace=False)
    cell = F.cells_of(xyz, G)[pick]
    want = F.direct_phi(xyz, w, EPS2, pick)
    dev = lambda got: np.abs(got - want) / np.abs(want)
    near = dev(F.phi64(lists, xyz, w, G, EPS2, xyz[pick], cell, pick, "flat", far=False))
    assert np.median(near) > 0.5                                     # (the far part is no small correction)
    for method in ("flat", "pyramid"):
        far = dev(F.phi64(lists, xyz, w, G, EPS2, xyz[pick], cell, pick, method))
        print("%s cloud, %d bodies on %d^3 cells, %s: far phi median %.3g max %.3g; stencil alone median %.3g max %.3g"
              % (kind, len(xyz), G, method, np.median(far), far.max(), np.median(near), near.max()))
        assert np.median(far) < np.median(near)


@pytest.mark.parametrize("method", ["flat", "pyramid"])
def test_the_two_forms_of_the_model_agree(method):
    """the fp32 association against the fp64 form, both signs of w; a kid among the points (w_eff 0: it sees every body)"""
    G = 8
    xyz, w, lists = cloud_frame("uniform", G, 4096)
    w = w.copy()
    w[::17] = 0.0
    pick = np.concatenate([np.arange(0, 170, 17), np.random.default_rng(14).choice(len(xyz), 190, replace=False)])
    cell = F.cells_of(xyz, G)[pick]
    for sign in (1.0, -1.0):
        a = F.phi64(lists, xyz, np.float32(sign) * w, G, EPS2, xyz[pick], cell, pick, method)
        b = F.phi32(lists, xyz, np.float32(sign) * w, G, EPS2, xyz[pick], cell, pick, method)
        rel = np.abs(b - a) / np.abs(a)
        print("%s, sign %+.0f: fp32 association against fp64, max %.3g" % (method, sign, rel.max()))
        assert b.dtype == np.float32 and (np.sign(a) == -sign).all() and rel.max() < F.ALLOW


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
