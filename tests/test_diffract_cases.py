"""The cases of tests/diffract_cases.py hold the classes they name -- on the CPU, from the reference alone (tests/diffract_ref.py), so that
the device comparison of tests/test_gpu_diffract.py is not a comparison of zeros."""
import numpy as np
import pytest

from tests import diffract_cases as dc


def seen(name):
    return dc.reference(dc.case_named(name))


def test_the_screen_has_shadowed_receivers_with_deposits_and_lit_ones_with_none():
    for case in dc.cases()[:6]:
        r = dc.reference(case)
        s = r["seen"]
        per = np.bincount(s["k"][s["deposited"]], minlength=case.K)
        assert s["blocked"].sum() >= 4 and (per[s["blocked"]] >= 1).all(), case.name             # every shadowed receiver gets a path
        lit = s["eligible"] & ~s["blocked"]
        assert lit.sum() >= 3 and not r["hist"][lit].any() and not r["det"][lit].any(), case.name   # a lit one gets nothing
        assert (np.bincount(s["k"], minlength=case.K)[lit] > 0).any()                               # ... although the search found pairs for it
        assert r["hist"].shape[-1] == (dc.CHANNELS[case.order] if case.order else case.B)
    assert {c.partition[0] for c in dc.cases()[:6]} == {"voxel", "octree", "kdtree"}
    assert {(c.B, c.order) for c in dc.cases()[:6]} >= {(1, 0), (3, 1), (8, 2), (3, 3)}


@pytest.mark.parametrize("name", ("wedge-B3", "wedge-B8-kdtree"))
def test_the_wedge_deposits_for_every_shadowed_receiver_over_edges_with_two_faces(name):
    case = dc.case_named(name)
    r = dc.reference(case)
    s = r["seen"]
    assert (case.faces >= 12).all() and case.faces.shape == (12, 2)
    per = np.bincount(s["k"][s["deposited"]], minlength=case.K)
    assert s["blocked"].sum() >= 4 and (per[s["blocked"]] >= 1).all() and r["hist"].any()


def test_the_numeric_edges_are_met():
    assert seen("edge-t0")["seen"]["t0"] == 1 and seen("edge-t0")["pairs"] == 1
    assert seen("edge-t1")["seen"]["t1"] == 1 and seen("edge-t1")["pairs"] == 1
    assert seen("edge-on-line")["seen"]["on_line"] == 1
    assert seen("edge-apex-in-sphere")["seen"]["in_sphere"] >= 1
    at, over = seen("edge-detour-at-limit"), seen("edge-detour-one-ulp-over")
    assert at["seen"]["at_limit"] == 1 and at["pairs"] == 1 and at["det"].sum() == 1
    assert over["seen"]["over_limit"] == 1 and over["pairs"] == 0
    assert seen("edge-detour-0")["pairs"] == 0 and seen("edge-detour-0")["seen"]["over_limit"] > 0
    assert 0 < seen("edge-detour-1m")["pairs"] < seen("screen-B1")["pairs"]
    lam = seen("edge-lambda-0-and-huge")
    assert (lam["seen"]["r"][:, 0] == 1.0 / 3.0).all() and (lam["seen"]["r"][:, 2] == 0.0).all()
    assert lam["hist"][..., 0].any() and not lam["hist"][..., 1].any() and not lam["hist"][..., 2].any()
    inside = seen("edge-source-in-receiver")["seen"]
    assert not inside["eligible"][1] and not (inside["k"] == 1).any()
    short = seen("edge-short-histogram")
    assert short["det"][:, 1].sum() > 0 and short["det"][:, 0].sum() > 0
    assert (seen("edge-directivity")["hist"] != seen("screen-B3-dir")["hist"]).any()


def test_the_sizes_cross_the_wave_and_the_tile():
    assert [dc.case_named(f"size-E{E}").ends.shape[0] for E in (1, 63, 65, 257)] == [1, 63, 65, 257]
    for name in ("size-K257-map", "size-K257-map-E65-dir"):
        case = dc.case_named(name)
        r = dc.reference(case)
        assert case.K == 257 and case.map and (r["seen"]["k"] == 256).any() and r["det"][256].sum() > 0      # the second tile's one receiver is in


def test_an_overflow_case_finds_more_pairs_than_its_list():
    assert dc.reference(dc.case_named("screen-B3-dir"))["pairs"] - 1 >= 1


def test_the_sweep_deposits_in_most_scenes():
    hit = sum(int(dc.reference(dc.sweep_case(seed))["det"].sum() > 0) for seed in dc.SWEEP)
    assert hit >= 25, hit
