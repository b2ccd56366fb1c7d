"""The far-field contexts' results are bit for bit what they were when tests/golden/far_bits.json was taken: the sorted order,
the force records and a far probe (acceleration and potential) on fixed small frames of both methods, and the exported state
after three steps with explosions.  scripts/far_bits.py builds the frames and forms the SHA-256 digests; the file names the
commit it was taken at and the command.  The other far tests hold flat against pyramid, probe against force record and model
against device; none of them can tell that an association is still the earlier one.  A digest that differs means the far walk
(or the sort, or the moments) computes other bits: the code is to be fixed, not the file."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import far_bits  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, "tests", "golden", "far_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_golden_file_holds_every_case():
    assert sorted(GOLDEN["cases"]) == sorted(far_bits.CASES) and len(GOLDEN["commit"]) == 40 and GOLDEN["commit"] in GOLDEN["command"]


@pytest.mark.parametrize("name", list(far_bits.CASES))
def test_digests_are_the_golden_ones(name):
    got, want = far_bits.digests_of(name), GOLDEN["cases"][name]
    differ = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    assert not differ, "%s: %s differ(s) from the bits taken at commit %s" % (name, ", ".join(differ), GOLDEN["commit"][:7])
