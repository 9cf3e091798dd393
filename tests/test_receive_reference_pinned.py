"""The receive loop's reference is pinned (no GPU).  tests.receive_ref.receive_loop defines the library's results bit for bit, so a
change to it -- three loops became one; the next feature is added to that one -- must be known to change nothing it should not.
tests/golden/receive_reference_digests.json holds tests.receive_cases.digest of what the three loops returned before they were merged,
for every fixed case of the four device modules, four rules' cases with the rules off (from the loop that did not know the rules), and
the sweeps' seeds; tests.receive_cases.reference must reproduce each.  The fixed cases' results are shared with the tests that need
them too (keep=True).  The plain sweep's seeds, all 200, are asserted where they are computed anyway
(tests/test_receive_cases.py::test_sweep_seeds_detect_something_within_the_size_bound); the rules' sweep has no such pass, so its 40
seeds are run here.  A digest that changes on purpose is a change of the specification: regenerate the file and say so."""
import pytest

from tests.receive_cases import digest, edge_cases, pinned_digests, reference
from tests.receive_cut_ref import cut_cases, sweep_cut_case
from tests.receive_map_ref import identity_cases, map_cases

CUT = cut_cases()
FIXED = ([("edge/", c) for c in edge_cases()] + [("cut/", c) for c in CUT] + [("map/", c) for c in map_cases()]
         + [("identity/", c) for c in identity_cases()]
         + [("rules-off/", c.without(time_limit=False, floor_bits=0, roulette=False)) for c in (CUT[1], CUT[12], CUT[16], CUT[17])])


def test_the_file_holds_exactly_the_cases():
    want = {kind + c.name for kind, c in FIXED} | {f"sweep/{s}" for s in range(200)} | {f"sweep-cut/{s}" for s in range(40)}
    assert set(pinned_digests()) == want


@pytest.mark.parametrize("kind,case", FIXED, ids=[kind + c.name for kind, c in FIXED])
def test_fixed_case_gives_the_pinned_result(kind, case):
    assert digest(reference(case, keep=True), per_cast=kind == "cut/") == pinned_digests()[kind + case.name], case.describe()


@pytest.mark.parametrize("seed", range(40))
def test_sweep_seed_with_the_rules_on_top_gives_the_pinned_result(seed):
    case = sweep_cut_case(seed)
    assert digest(reference(case), per_cast=True) == pinned_digests()[f"sweep-cut/{seed}"], case.describe()
