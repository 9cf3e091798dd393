"""What tests/test_gpu_receive_map_edges.py and tests/test_gpu_receive_map_sweep.py feed the library, proved by the restatement alone (no
GPU): every fixed case of tests.receive_map_ref.map_edge_cases() has a binned detection and went through the classes of the visit rule
it is there for (EXPECT, counted by candidates()' tallies); the set as a whole reaches every class; inside the header's domain
nothing is lost, and a map of K <= 256 receivers gives the bytes of the linear loop; every sweep seed has a binned detection and the
stated shares hold; every result is pinned in tests/golden/receive_map_reference_digests.json.

What no input can give: a detection that hangs on a padded face being inclusive, or on a ray that only touches the padded
grid: the points of such a ray are at least R = r_max + h / 8 from every center on that axis, a detection needs less than
r_k <= r_max.  The cases hold those rays and the rule gives them candidates; a histogram cannot tell.  The same holds for a skipped
slab (exact-skip builds one: a1 + P rounds up to an integer j while tA(j) > t1): its cells lie P from the segment's end.

The tie of the major axis: test_the_tie_break_changes_no_result runs the restatement with the tie given to the HIGHEST axis over the
edge set and finds the same bytes -- either major axis visits every cell a detection can lie in -- so no device test can fail on it."""
import json
import os

import numpy as np
import pytest

from tests.receive_cases import digest, reference
from tests.receive_map_ref import (DET_TALLIES, EXPECT, MAP_TALLIES, OUTSIDE, PAIRS_MAX, build_grid, candidates, candidates_tie_high, linear_detected, map_edge_cases,
                                   map_sweep_case)
from tests.receive_ref import receiver_step

SWEEP_SEEDS = 100                        # tests/test_gpu_receive_map_sweep.py's N
CASES = map_edge_cases()
UNREACHED = ()


def pinned():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "receive_map_reference_digests.json")) as f:
        return json.load(f)


def test_the_file_holds_exactly_the_cases():
    assert set(pinned()) == {"edge/" + c.name for c in CASES} | {f"sweep/{s}" for s in range(SWEEP_SEEDS)}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_fixed_case_holds_its_class_with_a_binned_detection(case):
    r = reference(case, keep=True)
    t = r["map_tallies"]
    print(case.describe(), {k: v for k, v in t.items() if v})
    assert r["det"][:, 0].sum() > 0 and r["hist"].any(), case.describe()
    for name in EXPECT[case.name]:
        assert t.get(name, 0) > 0, (case.name, name, t)
        if name + "_det" in DET_TALLIES:                                  # a per-ray class: rays OF THE CLASS hold detections
            assert t.get(name + "_det", 0) > 0, (case.name, name + "_det", t)
    assert case.n * case.K <= PAIRS_MAX and case.words <= 1 << 22
    if case.name not in OUTSIDE:
        assert t["lost"] == 0, (case.name, t)
    assert digest(r) == pinned()["edge/" + case.name], case.describe()


def test_the_edge_set_reaches_every_class_and_every_form():
    total = dict.fromkeys(MAP_TALLIES + DET_TALLIES, 0)
    for c in CASES:
        for k, v in reference(c, keep=True)["map_tallies"].items():
            total[k] += v
    print("edge set:", len(CASES), "cases; tallies", total)
    for name in MAP_TALLIES + DET_TALLIES:
        assert (total.get(name, 0) == 0) == (name in UNREACHED), (name, total)
    assert {(c.mode, c.directional) for c in CASES} == {(m, d) for m in ("specular", "scatter") for d in (False, True)}
    assert {c.partition[0] for c in CASES} == {"voxel", "octree", "kdtree"}
    assert {1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4159} <= {c.n for c in CASES} and {1, 3, 8} <= {c.B for c in CASES}
    assert {0, 1} == {c.pack for c in CASES if c.scene[0] == "soup" and c.n >= 4095}
    assert any(c.time_limit for c in CASES) and any(c.floor_bits and c.roulette for c in CASES)
    assert any(c.device for c in CASES) and any(c.two_scenes for c in CASES)
    cells = {c.name: build_grid(c.centers, c.radii, c.map_cell).dims.tolist() for c in CASES if c.name.startswith("cap-")}
    assert cells == {"cap-cube": [128, 128, 128], "cap-line": [1 << 21, 1, 1]}, cells


def test_the_exact_layout_is_exact_and_r2_is_strict():
    c = {x.name: x for x in CASES}
    g = build_grid(c["exact-axis"].centers, c["exact-axis"].radii, 0.0)
    assert g.h == 1.0 and g.pad == 0.625 and g.dims.tolist() == [10, 5, 2] and g.origin.tolist() == [1.0, 1.0, 1.0]
    x = c["exact-r2"]
    det = reference(x, keep=True)["det"].sum(axis=1)
    on = [k for k in range(x.K) if x.radii[k] == 0.25]
    inside = [k for k in range(x.K) if x.radii[k] == np.nextafter(0.25, 1.0)]
    assert len(on) == 1 and len(inside) == 1 and det[on[0]] == 0 and det[inside[0]] > 0, det     # q.q == r2 is no detection
    # the face rays of exact-axis hold candidates (the faces are inclusive), the rays one ulp beyond hold none
    rays = x = c["exact-axis"].rays
    cand = candidates(g, rays[:, :3], rays[:, 3:], np.full(rays.shape[0], 20.0))
    u = rays[:, :3] - 1.0
    on_face = ((rays[:, 3:] == 0) & ((u == -0.625) | (u == np.array([10.625, 5.625, 2.625])))).any(axis=1)
    beyond = ((rays[:, 3:] == 0) & ((u < -0.625) | (u > np.array([10.625, 5.625, 2.625])))).any(axis=1)
    assert on_face.sum() >= 24 and cand[on_face].any(axis=1).all() and beyond.sum() >= 12 and not cand[beyond].any()


def test_the_pairwise_test_is_the_receiver_steps():
    x = next(c for c in CASES if c.name == "exact-ties")
    o, d, t_end = x.rays[:, :3], x.rays[:, 3:], np.full(x.n, 3.0)
    det = np.zeros((x.K, 2), np.uint64)
    receiver_step(o, d, t_end, np.zeros(x.n), np.ones((1, x.n)), x.centers, x.radii, 4, 1.0, 0, np.zeros((x.K, 4, 1), np.uint64), det)
    assert np.array_equal(linear_detected(o, d, t_end, x.centers, x.radii).sum(axis=0), det.sum(axis=1).astype(np.int64))


IDENTITY = [c for c in CASES if c.name not in OUTSIDE and c.K <= 256]


@pytest.mark.parametrize("case", IDENTITY, ids=[c.name for c in IDENTITY])
def test_in_domain_map_equals_the_linear_loop(case):
    assert digest(reference(case, keep=True)) == digest(reference(case.without(map_cell=None), keep=True)), case.describe()


def test_sweep_seeds_detect_and_hold_the_stated_shares():
    above, rules, huge, forms, kinds, special = 0, 0, 0, set(), set(), 0
    for seed in range(SWEEP_SEEDS):
        c = map_sweep_case(seed)
        r = reference(c)
        assert r["det"][:, 0].sum() > 0, c.describe()
        assert digest(r) == pinned()[f"sweep/{seed}"], c.describe()
        assert r["map_tallies"]["lost"] == 0, c.describe()          # every seed, special values included: promise (a) wherever it applies
        assert c.words <= 1 << 22
        assert c.n * c.K <= PAIRS_MAX and 1 <= c.K <= 65536 and 1 <= c.bounces <= 4 and 1 <= c.B <= 8
        above += c.K > 256
        huge += c.K >= 16384
        rules += bool(c.time_limit or c.floor_bits)
        forms.add((c.mode, c.directional))
        kinds.add((c.scene[0], c.partition[0]))
        special += bool(np.isnan(c.rays).any())
    assert above >= SWEEP_SEEDS // 4 and huge == SWEEP_SEEDS // 20 and rules == SWEEP_SEEDS // 4, (above, huge, rules)
    assert len(forms) == 4 and {k[0] for k in kinds} == {"box", "shoebox", "room", "soup"} and {k[1] for k in kinds} == {"voxel", "octree", "kdtree"}
    assert special >= SWEEP_SEEDS // 10, special


def test_the_tie_break_changes_no_result():
    """The rule with a tie of the major axis given to the highest axis (candidates_tie_high: the rule on reversed axes): it chooses other
    candidates, and every case of the edge set that holds tied rays gives the digest of the rule as it stands."""
    tied = [c for c in CASES if any(reference(c, keep=True)["map_tallies"].get(k, 0) for k in ("tie_major_same", "tie_major_opposite"))]
    assert len(tied) >= 20
    x = next(c for c in CASES if c.name == "exact-ties")
    g = build_grid(x.centers, x.radii, 0.0)
    t_end = np.full(x.n, 2.0)
    plain, high = candidates(g, x.rays[:, :3], x.rays[:, 3:], t_end), candidates_tie_high(g, x.rays[:, :3], x.rays[:, 3:], t_end)
    untied = ~((np.abs(x.rays[:, 3]) == np.abs(x.rays[:, 4])) | (np.abs(x.rays[:, 4]) == np.abs(x.rays[:, 5])) | (np.abs(x.rays[:, 3]) == np.abs(x.rays[:, 5])))
    assert (plain != high).any() and untied.sum() > 20 and (plain[untied] == high[untied]).all()      # the variant differs on ties alone
    for c in tied:
        assert digest(reference(c, candidates_fn=candidates_tie_high)) == pinned()["edge/" + c.name], c.name
