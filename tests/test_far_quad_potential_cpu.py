"""PSAMD_POTENTIAL_QUADRUPOLE / PSAMD_PROBE_QUADRUPOLE without a GPU (test_far_model_cpu.py has the two bits,
psamd_download_potential_flags and the layouts that must not move): the keyword-only `quadrupole` of the four Python methods, the
potential's quadrupole term against the force term it must be the potential of, the METHOD against an fp64 direct sum over all
bodies, the model's two forms against each other (far_harness.py has the check, once for every method), and the limit in which
every C is an exact zero (far_model.py).

Measured with the seeds below, 8192 bodies, 400 sampled per cloud, median / maximum relative deviation of the far phi from the
direct sum -- pyramid; quadrupole; the ratio of the medians:
  8^3 uniform     1.76e-4 / 1.1e-3;  6.1e-5 / 2.9e-4;  0.35
  8^3 clustered   2.70e-4 / 1.1e-3;  1.12e-4 / 3.3e-4;  0.41
  10^3 uniform    1.08e-3 / 5.2e-3;  6.6e-5 / 3.1e-4;  0.06
  10^3 clustered  4.37e-4 / 2.9e-3;  1.07e-4 / 4.2e-4;  0.25
The central-difference gradient of the sum of t_q against far_model.quad_pull: 4.7e-10 relative at h = 1e-5.
The model's fp32 association against its fp64 form: 2.2e-7 (both signs; the quadrupole part is 2.8e-4 of |phi| for the median point)"""
import inspect

import numpy as np
import pytest

import far_model as F
import particlesystem_amd as ps
from far_harness import EPS2, low_corner, phi_against_the_direct_sum, two_forms_of_the_model_agree


# ---- 1. the C surface -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["potential", "download_potential", "energy", "probe"])
def test_quadrupole_is_keyword_only_and_off_by_default(name):
    p = inspect.signature(getattr(ps.ParticleSystem, name)).parameters
    assert p["quadrupole"].kind is inspect.Parameter.KEYWORD_ONLY and p["quadrupole"].default is False
    assert p["far"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and p["far"].default is False


# ---- 2. the formula ---------------------------------------------------------------------------------------------------------

def test_the_gradient_of_the_potential_term_is_the_force_term():
    """a = -grad phi and phi = -sum: a_q is the gradient of the sum of t_q.  Bodies at one to four cells' distance with random
    symmetric second moments, central differences at h = 1e-5 in fp64: the truncation is of the order h^2 / r^2 = 1e-12, the
    rounding 1e-16 / h relative = 1e-11"""
    rng = np.random.default_rng(3)
    bodies = rng.uniform(-20.0, 20.0, (40, 3))
    a = rng.normal(0.0, 1.5, (40, 3, 3))
    cen = np.stack([np.einsum("bki,bkj->bij", a, a)[:, i, j] * 60.0 for i, j in F.PLANES], 1)
    at = rng.uniform(-2.5, 2.5, (25, 3))
    h = 1e-5
    grad = np.zeros((len(at), 3))
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        grad[:, k] = (F.quad_terms64(at + e, bodies, cen, EPS2).sum(1) - F.quad_terms64(at - e, bodies, cen, EPS2).sum(1)) / (2 * h)
    want = F.quad_pull(at, bodies, cen, EPS2)
    rel = F.rel_dev(grad, want)
    print("central-difference gradient of the sum of t_q against quad_pull: max %.3g relative" % rel.max())
    assert np.linalg.norm(want, axis=1).min() > 0 and rel.max() < 1e-6


# ---- 3. the method ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [8, 10])
@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_the_method_against_the_direct_sum(kind, G):
    dev = phi_against_the_direct_sum(kind, G)
    pyr, quad = dev["pyramid"], dev["quadrupole"]
    print("%s cloud, 8192 bodies on %d^3 cells: far phi as a pyramid median %.3g max %.3g; with quadrupoles median %.3g max %.3g; "
          "ratio of the medians %.2f" % (kind, G, np.median(pyr), pyr.max(), np.median(quad), quad.max(), np.median(quad) / np.median(pyr)))
    assert np.median(quad) <= 0.5 * np.median(pyr)


# ---- 4. the model's two forms -----------------------------------------------------------------------------------------------

def test_the_two_forms_of_the_model_agree():
    two_forms_of_the_model_agree("quadrupole")


# ---- 5. every C an exact zero -------------------------------------------------------------------------------------------------

def test_one_adult_a_cell_is_the_pyramid_phi():
    """4^3 cells with one adult each and 300 kids anywhere: both products of C_ab round the same real number, so every C is an
    exact zero, every quadrupole chain +0, and the fp32 form is the pyramid's to the bit"""
    G = 4
    rng = np.random.default_rng(5)
    adults = np.array([low_corner(i1, i2, i3, G) for i3 in range(G) for i1 in range(G) for i2 in range(G)]) + rng.uniform(0.1, 4.9, (G ** 3, 3))
    kids = rng.uniform(-9.9, 9.9, (300, 3))
    xyz = np.concatenate([adults, kids]).astype(np.float32)
    w = np.concatenate([rng.uniform(20.0, 100.0, G ** 3), np.zeros(300)]).astype(np.float32)
    lists = F.lists_of(xyz, G)
    cell = F.cells_of(xyz, G)
    idx = np.arange(len(xyz))
    moments = F.level_moments(lists, xyz, w, G, "quadrupole")
    assert len(moments[1]) == 1 and not moments[1][0].any() and (moments[0][0][:, 3] != 0).all()
    got = F.phi32(lists, xyz, w, G, EPS2, xyz, cell, idx, "quadrupole", moments)
    want = F.phi32(lists, xyz, w, G, EPS2, xyz, cell, idx, "pyramid", (moments[0], None))
    assert np.array_equal(got, want) and np.abs(got).min() > 0
