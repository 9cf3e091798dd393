"""The receive loop on the MI355X over a seeded sweep of its whole parameter space: tests.receive_cases.sweep_case(seed) for seeds
0 .. N - 1 -- random soups with quadrilaterals, the shoebox and the partition room; the three partitions with drawn parameters; 1 to
about 20 000 rays, weighted towards multiples of 64 +- 1 and the live-block list's threshold; 1 .. 8 casts, K = 1 .. 256, B = 1 .. 8,
tables with rows of 0 and 1, the six kernel forms, the aggregated and the per-lane add, bounce_pack, frac_bits 0 .. 62, 1 .. 2000 bins
of 1 mm .. 10 m, a starting state or none, scatter seeds over the whole int64 range, one partition or two through the sharded call.
Compared with the numpy restatement as tests/test_gpu_receive_edges.py compares.  No seed is skipped or redrawn
(tests/test_receive_cases.py: each detects something).  tools/fuzz_receive.py runs the same cases over any seed range.

N = 200.  The reference side of these seeds takes about 150 s on a 16-thread CPU host.  On an MI355X host the whole module, reference
side included, takes 37 s of wall time (200 passed; 16 threads of a faster CPU; 38 s before tests/receive_harness.py took over the
device side)."""
import pytest

from tests.receive_cases import reference, sweep_case
from tests.receive_harness import check_case

pytestmark = pytest.mark.gpu

N = 200


@pytest.mark.parametrize("seed", range(N))
def test_sweep_seed_equals_the_reference(seed):
    case = sweep_case(seed)
    want = reference(case)
    assert want["det"].sum() > 0, case.describe()
    bad = check_case(case, want)
    assert bad is None, (case.describe(), bad, {k: v for k, v in want["tallies"].items() if v})
