"""The source paths on the MI355X at their numeric edges, in oblique rooms: every case of tests.path_cases.edge_cases() -- P about a block
and a tile of 256 polygons, K about 256; d2 one ulp either side of rr and on it, per order; the source in an oblique polygon's plane and
one ulp off it; coplanar neighbours in an oblique plane; the prune's limits; the pre-cull's limits; leave directions on the cube map's
edges and corners -- through tests.path_harness.check_case against tests.path_cases.reference: histogram and detections byte for byte,
the counts, the lists as sets, the guards, the HIP call counters.  A case that carries an option pair ("image_cull", "image2_prune") runs
with 0 and with 1, and both must equal the reference.  tests/test_path_cases.py asserts on the CPU that each case holds the class it
names."""
import pytest

from tests.path_cases import edge_cases, reference, variants
from tests.path_harness import check_case

pytestmark = pytest.mark.gpu

RUNS = [v for c in edge_cases() for v in variants(c)]


@pytest.mark.parametrize("case", RUNS, ids=[c.name + "".join(f"-{o.split('_')[1]}{getattr(c, o)}" for o in c.pair) for c in RUNS])
def test_edge_case_equals_the_reference(case):
    want = reference(case, keep=True)                                   # the options do not enter the reference: one result per name
    bad = check_case(case, want)
    assert bad is None, (case.describe(), case.why, bad)
