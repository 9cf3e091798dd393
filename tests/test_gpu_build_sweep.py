"""The GPU partition builders on the MI355X over a seeded sweep: tests.build_cases.sweep_case(seed) for seeds 0 .. N - 1 -- the degenerate
mix (zero-area and repeated-corner polygons, slivers, corners and whole polygons exactly on a cell plane and in a padded face, polygons
across the whole grid) at scales of 10^-3 .. 10^3, sometimes far from the origin, P = 40 .. 3000, one or two topologies; a fixed grid of
D in {1, 2, 3, 7, 12, 13, 31, 40}, an adaptive grid of max_domain up to 5 or an octree of depth up to 7.  Compared with the oracle as
tests/test_gpu_build_edges.py compares: `built_on_device`, lists or node arrays, `ct`, boxes and dimensions equal, a second build equal
byte for byte, and for a grid one shoot per topology.  No seed is skipped or redrawn; tests/test_build_cases.py pins every seed's
reference.  tools/fuzz_builders.py runs the same cases over any seed range."""
import pytest

from tests.build_cases import check_case, reference, sweep_case

pytestmark = pytest.mark.gpu

N = 24


@pytest.mark.parametrize("seed", range(N))
def test_sweep_seed_equals_the_oracle(seed, monkeypatch):
    monkeypatch.delenv("HARE_BUILD", raising=False)
    case = sweep_case(seed)
    bad = check_case(case, reference(case))
    assert bad is None, (case.describe(), case.why, bad)
