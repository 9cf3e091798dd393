"""The receive loop's termination rules on the MI355X (include/hare_hip.h, "receivers", "Termination"): the time limit
(HARE_RECEIVE_TIME_LIMIT), the energy floor ("receive_floor_bits") and its roulette ("receive_roulette").  Every case of
tests.receive_cut_ref.cut_cases() -- each rule alone and all together, in the six kernel forms, on the three partitions, at batch sizes
about a wave, a workgroup and the live-block list's threshold, with bounce_pack and receive_aggregate on and off, from a starting state
with L past the end, infinities and NaN, and in an open room where rays also retire by missing -- through Receive_batch and, for a
subset, through receive_device on the caller's buffers.  Histogram, detections and final state (for the device call also the rays and
the last events) equal the numpy restatement (tests/receive_ref.py) byte for byte; of a NaN only that it is one is compared.
tests/test_receive_cut_api.py proves with the restatement alone that the cases are not vacuous.  Further: the time-limit call's
histogram and binned detections are those of the call without the flag; the sharded call over two scenes equals the one-scene call
(the roulette draws on global ray indices); forty seeds of the receive sweep with the rules drawn on top."""
import pytest

from tests.receive_cases import reference
from tests.receive_cut_ref import cut_cases, sweep_cut_case
from tests.receive_harness import check_case, library_partitions, mismatch, run_batch, same_bits

pytestmark = pytest.mark.gpu

CASES = cut_cases()
SWEEP_SEEDS = 40


@pytest.mark.parametrize("cc", CASES, ids=[c.name for c in CASES])
def test_case_equals_the_reference(cc):
    want = reference(cc, keep=True)
    assert want["det"][:, 0].sum() > 0, cc.describe()
    bad = check_case(cc, want)
    assert bad is None, (cc.describe(), bad, {k: v.tolist() for k, v in want["per_cast"].items()})


@pytest.mark.parametrize("cc", [c for c in CASES if c.time_limit and c.n >= 4097], ids=lambda c: c.name)
def test_the_time_limit_changes_neither_histogram_nor_binned_detections_on_the_device(cc):
    parts = library_partitions(cc)
    h1, d1, s1 = run_batch(cc, parts, time_limit=True)
    h0, d0, s0 = run_batch(cc, parts, time_limit=False)
    assert h1.any()
    assert same_bits(h1, h0) is None and same_bits(d1[:, 0], d0[:, 0]) is None
    assert d1[:, 1].sum() < d0[:, 1].sum()              # the flag was not ignored: the retired rays' unbinned detections are gone
    assert same_bits(s1, s0) is not None


@pytest.mark.parametrize("cc", [c for c in CASES if c.name in ("roulette-4159", "all-4159", "all-state", "floor-4097")], ids=lambda c: c.name)
def test_two_scenes_on_one_device_equal_the_one_scene_call(cc):
    want = reference(cc, keep=True)
    hist, det, state = run_batch(cc, library_partitions(cc, count=2))
    bad = mismatch(want, hist, det, state)
    assert bad is None, (cc.describe(), bad)


@pytest.mark.parametrize("seed", range(SWEEP_SEEDS))
def test_sweep_seed_with_the_rules_on_top_equals_the_reference(seed):
    cc = sweep_cut_case(seed)
    want = reference(cc)
    bad = check_case(cc, want, device=seed % 4 == 0)
    print(cc.describe(), {k: int(v.sum()) for k, v in want["per_cast"].items()})
    assert bad is None, (cc.describe(), bad, {k: v.tolist() for k, v in want["per_cast"].items()})
