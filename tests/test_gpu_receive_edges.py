"""The receive loop on the MI355X at the numeric edges of its definition (include/hare_hip.h, "receivers"): every case of
tests.receive_cases.edge_cases() -- states full of NaN, infinities, negative values, signed zeros, denormals, ties and values that
saturate at 2^63 or clamp at +-2^62; sums that wrap; L exactly on a bin edge and at n_bins; B = 1 .. 8; K = 1, 64, 255, 256; batch
sizes about a wave, a workgroup and the live-block list's threshold; one bin, and a wave's lanes in distinct bins; exclusions on the
first cast; lanes whose arrival vector is not a number beside lanes that deposit -- through Receive_batch, and a subset through
receive_device with the caller's buffers.  Histogram, detections, final state (and, for the device call, rays and last events) equal
the numpy restatement (tests/receive_ref.py) byte for byte; of a NaN only that it is one is compared (its sign and payload are the FPU's,
DESIGN.md 1).  A directional call's channel 0, detections and state are those of the call without the flag (tests/receive_harness.py:
check_case, the one comparison of the four receive modules).
tests/test_receive_cases.py proves, with the reference alone, that the cases hold these classes."""
import pytest

from tests.receive_cases import edge_cases, reference
from tests.receive_harness import check_case

pytestmark = pytest.mark.gpu

CASES = edge_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_edge_case_equals_the_reference(case):
    want = reference(case, keep=True)
    assert want["det"].sum() > 0, case.describe()
    bad = check_case(case, want)
    print(case.describe(), "tallies", {k: v for k, v in want["tallies"].items() if v})
    assert bad is None, (case.describe(), bad, {k: v for k, v in want["tallies"].items() if v})


def test_the_device_subset_holds_small_batches_and_the_threshold():
    ns = {c.n for c in CASES if c.device}
    assert any(n < 4096 for n in ns) and 4096 in ns and any(n < 256 for n in ns), ns
