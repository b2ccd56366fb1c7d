"""PSAMD_FLAG_FAR_MONOPOLE without a GPU (test_far_model_cpu.py has the flag and the entry point): the METHOD -- the stencil as a direct sum, every other cell as one monopole (far_model.py, "flat") --
against an fp64 direct sum over all bodies.  The caps (median 5e-3, maximum 5e-2, the stencil alone above 0.5) are a
property of the method, not of the device code.  Measured with the seeds below, 400 particles sampled per cloud: median /
maximum relative deviation of |a| 2.1e-3 / 3.5e-2 on the uniform cloud and 1.5e-3 / 1.6e-2 on the clustered one; the
stencil alone: median 0.87 and 0.77."""
import numpy as np
import pytest

import far_model as F
from far_harness import method_against_the_direct_sum


@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_the_method_against_the_direct_sum(kind):
    far, near = method_against_the_direct_sum("flat", kind, 8)
    assert np.median(far) < 5e-3
    assert far.max() < 5e-2
    assert np.median(near) > 0.5


def test_the_moments_of_a_hand_made_frame():
    """one adult: its own position and mass, exactly; kids only: zeros; the centre of mass of two; repulsion flips M alone"""
    xyz = np.array([[1.25, -2.5, 3.0], [7.0, 7.0, 7.0], [6.0, 8.0, 9.0], [-12.0, 1.0, 1.0], [-13.0, 2.0, 1.5]], np.float32)
    w = np.array([60.0, 0.0, 0.0, 20.0, 60.0], np.float32)
    lists = [np.array([0]), np.array([1, 2]), np.array([3, 4]), np.array([], np.int64)]
    # a cell's moments depend on its own list alone, not on where the cell lies: the four lists are given as the first four
    # cells of the smallest frame that holds them, 2^3 cells, the other four empty
    moments = lambda w: F.level_moments(lists + [np.array([], np.int64)] * 4, xyz, w, 2, "flat")[0][0][:4]
    m = moments(w)
    assert m[0].tolist() == [1.25, -2.5, 3.0, 60.0]
    assert not m[1].any() and not m[3].any()
    assert m[2].tolist() == [np.float32((20.0 * -12.0 + 60.0 * -13.0) / 80.0), 1.75, np.float32((20.0 + 90.0) / 80.0), 80.0]
    r = moments(-w)
    assert np.array_equal(r[:, :3], m[:, :3]) and np.array_equal(r[:, 3], -m[:, 3])
