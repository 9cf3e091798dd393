"""What tests/test_gpu_receive_edges.py and tests/test_gpu_receive_sweep.py feed the library, proved by the reference alone (no GPU): over
the edge set every class of the definition's awkward cases occurs (tests.receive_ref.TALLIES) and so does every shape the kernels treat
differently; every sweep seed detects something, stays within the histogram's size bound and gives the result whose digest
tests/golden/receive_reference_digests.json pins (tests/test_receive_reference_pinned.py holds the other cases).  Without this a device
test could pass on inputs that never reach the code it is there for.

One class cannot occur in any deposit: a directional word zeroed for NaN.  m is never NaN (it is 0 unless > 0) and a deposit's arrival
vector is finite: a = -(d / len) needs len = 0 or inf, i.e. dd = 0 or inf, and then s = (w.d) / dd is NaN, +-inf or 0 / inf with a
non-finite len only through an infinite d -- never s >= 0 && s < t_end with a NaN quotient; in the rain dist = sqrt(d2) with
inf > d2 > rr > 0.  The branch still matters on the device: in the aggregated add EVERY lane of the wave feeds the butterfly, a lane
that deposits nothing with m = 0 and its own arrival vector, and 0 * NaN (or 0 * inf) must give the word 0.  So the tally is asserted
to stay 0 and the edge set is asserted to hold such lanes (a direction scaled by 2^-600: dd underflows to 0) beside depositing ones."""
import numpy as np

from tests.receive_cases import MODES, WORDS_MAX, digest, edge_cases, pinned_digests, reference, sweep_case, wave_counts
from tests.receive_ref import TALLIES, signed_words

SWEEP_SEEDS = 200                        # tests/test_gpu_receive_sweep.py's N


def test_edge_set_holds_every_class_and_every_shape():
    cases = edge_cases()
    total = dict.fromkeys(TALLIES, 0)
    binned = unbinned = 0
    forms, rain_seen, room_occlusion = set(), False, False
    for c in cases:
        r = reference(c, keep=True)
        assert r["det"].sum() > 0, c.describe()
        for k, v in r["tallies"].items():
            total[k] += v
        binned += int(r["det"][:, 0].sum())
        unbinned += int(r["det"][:, 1].sum())
        forms.add((c.mode, c.directional, c.aggregate))
        if c.mode == "rain":
            assert r["stats"]["eligible"] > 0, c.describe()
            rain_seen = True
            if c.scene == ("room",) and 0 < r["stats"]["occluded"] < r["stats"]["eligible"]:
                room_occlusion = True
    print("edge set:", len(cases), "cases; tallies", total, "binned", binned, "not binned", unbinned)
    for name in TALLIES:
        if name != "dir_nan":
            assert total[name] > 0, (name, total)
    assert total["dir_nan"] == 0, total                                  # see the module's docstring
    assert binned > 0 and unbinned > 0
    assert forms == {(m, d, a) for m in MODES for d in (False, True) for a in (1, 0)}, forms
    assert rain_seen and room_occlusion
    assert {c.B for c in cases if not c.directional and c.aggregate} == set(range(1, 9))     # the lane map lane == b
    assert {c.B for c in cases if c.directional and c.aggregate} == set(range(1, 9))         # the lane map (lane & 15) == b
    assert {1, 64, 255, 256} <= {c.K for c in cases}
    assert {1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097} <= {c.n for c in cases}
    assert {0, 1, 62} == {c.frac_bits for c in cases} and {1, 2} == {c.bounces for c in cases}
    assert any(c.n_bins == 1 for c in cases) and any(c.excl1 is not None and c.excl2 is not None for c in cases)
    assert all(c.words <= WORDS_MAX for c in cases)


def test_edge_set_has_a_wave_in_distinct_bins_and_a_wave_in_one_bin():
    cases = {c.name: c for c in edge_cases()}
    for name in ("distinct-bins-0", "distinct-bins-1"):
        c = cases[name]
        assert c.aggregate == 1
        most = max(int(np.count_nonzero(wave_counts(c, w)[0])) for w in range(0, c.n // 64, 7))
        print(name, "most distinct bins of receiver 0 in one wave's first cast:", most)
        assert most >= 48, (name, most)
    for name in ("one-bin-0", "one-bin-1"):
        c = cases[name]
        cnt = wave_counts(c, 1)
        assert c.aggregate == 1 and cnt.shape[1] == 1 and cnt[0, 0] >= 2, (name, cnt)


def test_edge_set_has_lanes_without_an_arrival_vector_beside_depositing_lanes():
    for c in (c for c in edge_cases() if c.name.startswith("tiny-")):
        assert c.directional and c.mode == "specular"
        d = c.rays[:, 3:]
        with np.errstate(under="ignore"):
            dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        odd = np.nonzero(dd == 0)[0]
        assert odd.size >= c.n // 64 and np.all(odd % 64 == 17)
        with np.errstate(all="ignore"):
            a = -(d[odd] / np.sqrt(dd[odd])[:, None])
            assert not np.isfinite(a).any()                              # -(d / 0): infinities (and NaN for a zero component)
            assert not np.isfinite(0.0 * a).any()                        # m = 0 of a lane that deposits nothing: 0 * inf = NaN
        assert np.all(signed_words(np.float64(0.0), a[:, 0]) == 0)       # the word the definition gives it
        cnt = wave_counts(c, int(odd[3]) // 64)
        assert cnt.sum() >= 32, cnt.sum()                                # the same wave deposits
    assert {c.aggregate for c in edge_cases() if c.name.startswith("tiny-")} == {0, 1}


def test_sweep_seeds_detect_something_within_the_size_bound():
    kinds, modes, shards, small = set(), set(), set(), 0
    for seed in range(SWEEP_SEEDS):
        c = sweep_case(seed)
        r = reference(c)
        assert r["det"].sum() > 0, c.describe()
        assert digest(r) == pinned_digests()[f"sweep/{seed}"], c.describe()       # the one pass over the seeds serves the pin too
        assert c.words <= WORDS_MAX and 1 <= c.K <= 256 and 1 <= c.B <= 8 and 1 <= c.bounces <= 8 and 0 <= c.frac_bits <= 62
        kinds.add((c.scene[0], c.partition[0]))
        modes.add((c.mode, c.directional, c.aggregate))
        shards.add(c.shards)
        small += c.n < 256
    assert len(kinds) == 9 and len(modes) == 12 and shards == {1, 2} and small > 0
