"""Receiver maps on the MI355X over a seeded sweep: tests.receive_map_ref.map_sweep_case(seed) for seeds 0 .. N - 1 -- the six map
layouts and the degenerate grids, K = 1 .. 65 536, a caller's cell of 1/16 .. 64 of the diameter, rooms scaled by 2^-10 .. 2^10 per
axis and shifted by up to 2^19 cells, axis-parallel, diagonal, grazing and scaled rays, one seed in five sprinkled with NaN, infinities,
zeros and denormals, 1 .. 4 casts, the four _map kernels, the three partitions, B = 1 .. 8, frac_bits 0 .. 62, bounce_pack, the
termination rules in a quarter of the seeds, a starting state or none, one scene or two.  Compared as tests/test_gpu_receive_map_edges.py
compares; inside the header's domain a map of K <= 256 receivers also gives the bytes of set_receivers (a seed with special values or
lost pairs is outside it).  No seed is skipped or redrawn (tests/test_receive_map_cases.py: each has a binned detection).
tools/fuzz_receive.py with MAP=1 runs the same cases over any seed range."""
import numpy as np
import pytest

from tests.receive_cases import reference
from tests.receive_harness import check_case, library_partitions, mismatch, run_batch
from tests.receive_map_ref import map_sweep_case

pytestmark = pytest.mark.gpu

N = 100


@pytest.mark.parametrize("seed", range(N))
def test_map_sweep_seed_equals_the_reference(seed):
    case = map_sweep_case(seed)
    want = reference(case)
    assert want["det"][:, 0].sum() > 0, case.describe()
    bad = check_case(case, want, device=seed % 4 == 0)
    assert bad is None, (case.describe(), bad, {k: v for k, v in want["map_tallies"].items() if v})
    if case.K <= 256 and np.isfinite(case.rays).all() and want["map_tallies"]["lost"] == 0:
        hist, det, state = run_batch(case, library_partitions(case, linear=True))
        bad = mismatch(want, hist, det, state)
        assert bad is None, (case.describe(), "set_receivers " + bad)
