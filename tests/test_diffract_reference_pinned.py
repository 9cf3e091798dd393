"""tests/diffract_ref.py pinned: the digest of what the reference returns (histogram, detections, pair count) for every fixed case of
tests/diffract_cases.py and every seed of its sweep is the one in tests/golden/diffract_reference_digests.json, so the yardstick of
tests/test_gpu_diffract.py cannot drift unseen.  `python -m tests.test_diffract_reference_pinned --record` (from the repository's root) writes the file; it is written
from the reference alone, never from the library."""
import json
import os
import sys

import pytest

from tests import diffract_cases as dc

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diffract_reference_digests.json")


def all_cases():
    return dc.cases() + [dc.sweep_case(seed) for seed in dc.SWEEP]


def test_the_fixture_names_every_case():
    assert sorted(json.load(open(FIXTURE))) == sorted(c.name for c in all_cases())


@pytest.mark.parametrize("case", all_cases(), ids=lambda c: c.name)
def test_the_reference_is_the_pinned_one(case):
    assert dc.digest(dc.reference(case)) == json.load(open(FIXTURE))[case.name]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    json.dump({c.name: dc.digest(dc.reference(c)) for c in all_cases()}, open(FIXTURE, "w"), indent=1, sort_keys=True)
