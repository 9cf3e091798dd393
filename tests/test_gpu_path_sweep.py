"""The source paths on the MI355X over a seeded sweep of their whole parameter space: tests.path_cases.sweep_case(seed) for seeds
0 .. N - 1 -- tessellated shoeboxes, the box of quadrilaterals, the baffle room and the partition room, with and without occluders from
tests.helpers.soup, rotated by a drawn quaternion, scaled per axis by 0.6 .. 1.7 and moved by up to 1000 m; the three partitions with
drawn parameters; K = 1 .. 300, weighted towards 1, 8 and 255 .. 257, a map above 256 and sometimes below; B = 1 .. 8; R = 0, 1, 4 in a
drawn frame; tables none / alpha / alpha+sigma with rows of 0 and of 1; frac_bits 0 .. 62; 1 .. 2000 bins of 1 mm .. 10 m; one or four
channels; n_weight 1, 4 097, 2^40; any non-empty subset of the three orders; "image_cull" and "image2_prune" 0 or 1.  Compared with the
numpy restatements as tests/test_gpu_path_edges.py compares.  No seed is skipped or redrawn (tests/test_path_cases.py: each deposits
something).  tools/fuzz_paths.py runs the same cases over any seed range.

N = 100.  On an MI355X host this module alone, reference side included, takes 14.2 s of wall time (100 passed; 16 threads).  The cap
K x P x P <= 1 000 000 where the second order runs keeps the reference side of these seeds at about 40 s on a slow 16-thread CPU host (65 s
at 4 000 000)."""
import pytest

from tests.path_cases import reference, sweep_case
from tests.path_harness import check_case

pytestmark = pytest.mark.gpu

N = 100


@pytest.mark.parametrize("seed", range(N))
def test_sweep_seed_equals_the_reference(seed):
    case = sweep_case(seed)
    want = reference(case)
    assert sum(int(w["det"].sum()) for w in want.values()) > 0, case.describe()
    bad = check_case(case, want)
    assert bad is None, (case.describe(), bad)
