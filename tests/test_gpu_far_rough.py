"""The far field off the tame frames (include/psamd.h, "long-range gravity", "a pyramid of monopoles", "quadrupoles on the pyramid"):
the device against the numpy model (far_model.py) where the other far suites never go -- grids of four and five levels, collisions
at the default radius, clumps, repulsion in the force records.  The checks are far_force_suite.py's (section 7: their bodies,
docstrings and what can go wrong there) and three of far_field_suite.py's at the deep grids; the clouds, grid rows and frames are
far_harness.py's (DEEP, rough_bodies, rough_frame).  Every numeric bar is one the suites had: REL = 1e-5, and the reused
checks' own.  What was measured on an MI355X stands in CHANGELOG.md."""
import pytest

pytest.register_assert_rewrite("far_force_suite")       # (its asserts are this suite's: show their operands)

import far_field_suite as V  # noqa: E402
import far_force_suite as S  # noqa: E402
from far_harness import DEEP  # noqa: E402

pytestmark = pytest.mark.gpu

METHODS = ("flat", "pyramid", "quadrupole")
# pyramid and quadrupole on every deep grid; flat on 20^3 alone (125 blocks over 16 parts; its cost grows with G^3)
DEEP_CASES = [pytest.param(m, G, id="%s-%d^3" % (m, G)) for G in DEEP for m in METHODS if m != "flat" or G == 20]
SERVICE_CASES = [pytest.param(m, G, id="%s-%d^3" % (m, G)) for G in (24, 36) for m in ("pyramid", "quadrupole")]


# ---- 1. deep pyramids ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method,G", DEEP_CASES)
def test_deep_moments_equal_the_model_bit_for_bit(method, G):
    S.deep_moments_equal_the_model_bit_for_bit(method, G)


@pytest.mark.parametrize("method,G", DEEP_CASES)
def test_deep_force_records_follow_the_model(method, G):
    S.deep_force_records_follow_the_model(method, G)


def test_fast_math_on_five_levels_follows_the_model_and_gives_the_same_bytes_twice():
    """quadrupoles on 36^3"""
    S.deep_force_records_follow_the_model("quadrupole", 36, S.ps.FLAG_FAST_MATH)


# ---- 2. the services on a deep grid ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method,G", SERVICE_CASES)
def test_acc_probes_on_served_adults_are_their_force_records_bit_for_bit(method, G):
    V.acc_probes_on_served_adults_are_their_force_records_bit_for_bit(method, G)


@pytest.mark.parametrize("method,G", SERVICE_CASES)
def test_phi_probes_on_kids_are_the_kids_phi_bit_for_bit(method, G):
    V.phi_probes_on_kids_are_the_kids_phi_bit_for_bit(method, G)


@pytest.mark.parametrize("method,G", SERVICE_CASES)
def test_phi_and_U_follow_the_model(method, G):
    V.phi_and_U_follow_the_model(method, G, 1.0)


# ---- 3. collisions, 4. clumps, 5. repulsion ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", METHODS)
def test_collisions_at_the_default_radius(method):
    S.collisions_at_the_default_radius(method)


@pytest.mark.parametrize("kind", ["clump", "rough"])
@pytest.mark.parametrize("method", METHODS)
def test_clumps_follow_the_model_whole_and_in_the_far_part(method, kind):
    S.clumps_follow_the_model_whole_and_in_the_far_part(method, kind)


@pytest.mark.parametrize("G", [8, 10], ids=lambda G: "%d^3" % G)
@pytest.mark.parametrize("method", METHODS)
def test_repulsion_in_the_force_records(method, G):
    S.repulsion_in_the_force_records(method, G)


for _test in (test_deep_moments_equal_the_model_bit_for_bit, test_deep_force_records_follow_the_model, test_collisions_at_the_default_radius,
              test_clumps_follow_the_model_whole_and_in_the_far_part, test_repulsion_in_the_force_records):
    _test.__doc__ = getattr(S, _test.__name__[5:]).__doc__
