"""The higher-order receivers on the MI355X over a seeded sweep: tests.ambi_cases.sweep_case(seed) for seeds 0 .. 49 -- the cases of
tests/test_gpu_receive_sweep.py (scenes, partitions, n, casts, K, B, tables, modes, the aggregated and the per-lane add, frac_bits, bins,
starting states, one partition or two) with HARE_RECEIVE_DIRECTIONAL on, an order of 2 or 3 drawn from the seed, and every third
(but never with rain) through a receiver map over the same receivers.  Compared byte for byte with tests/ambi_ref.py as
tests/test_gpu_ambi.py compares; the reference's digests are pinned in tests/golden/ambi_reference_digests.json
(tests/test_ambi_reference.py).  No seed is skipped or redrawn."""
import pytest

from tests import ambi_cases as ac
from tests.ambi_harness import check_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", ac.SWEEP_SEEDS)
def test_sweep_seed_equals_the_reference(seed):
    case = ac.sweep_case(seed)
    want = ac.reference(case)
    bad = check_case(case, want, device=seed % 5 == 0)
    assert bad is None, (case.describe(), bad)
