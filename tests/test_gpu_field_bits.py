"""What tests/golden/far_bits.json does not pin is bit for bit what it was when tests/golden/field_bits.json was taken: the force
records and far probes of quadrupole contexts (acceleration and potential together and each alone), psamd_potential's phi in
export order and its result record in every form (cutoff, lists longer than one chain, all-pairs, flat, pyramid, quadrupoles),
probes of all-pairs and cutoff contexts (lean exact, fast and generic exact arithmetic) and the exported state after three steps
with explosions on a quadrupole context.  scripts/field_bits.py builds the frames and forms the SHA-256 digests; the file names
the commit it was taken at and the command.  A digest that differs means that a walk over the field (the stencil lookup, a
cell walk, the moments, a far block) computes other bits: the code is to be fixed, not the file."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import field_bits  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, "tests", "golden", "field_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_golden_file_holds_every_case():
    assert sorted(GOLDEN["cases"]) == sorted(field_bits.CASES) and len(GOLDEN["commit"]) == 40 and GOLDEN["commit"] in GOLDEN["command"]


@pytest.mark.parametrize("name", list(field_bits.CASES))
def test_digests_are_the_golden_ones(name):
    got, want = field_bits.digests_of(name), GOLDEN["cases"][name]
    differ = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    assert not differ, "%s: %s differ(s) from the bits taken at commit %s" % (name, ", ".join(differ), GOLDEN["commit"][:7])
