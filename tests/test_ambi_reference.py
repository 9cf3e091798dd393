"""The higher-order receivers (include/hare_hip.h, "receivers", "Higher orders") without a GPU: the numpy restatement
(tests/ambi_ref.py) against what is known of the harmonics -- the constants, known answers, the SN3D identity, the nesting of the orders
-- its results on the fixed cases and the sweep pinned by digest (tests/golden/ambi_reference_digests.json), and the calls' first check:
the order flags without HARE_RECEIVE_DIRECTIONAL, both at once, and the histogram cap at sixteen channels."""
import os
import re

import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests import ambi_cases as ac
from tests import ambi_ref
from tests import receive_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECEIVE_HIP = os.path.join(ROOT, "hare_amd", "csrc", "receive.hip")
O2, O3, DIR = capi.RECEIVE_ORDER2, capi.RECEIVE_ORDER3, capi.RECEIVE_DIRECTIONAL


# ---- the constants
WANT = {"c3": np.sqrt(np.float64(3.0)), "c3h": np.float64(0.5) * np.sqrt(np.float64(3.0)), "c15": np.sqrt(np.float64(15.0)),
        "c15h": np.float64(0.5) * np.sqrt(np.float64(15.0)), "c58": np.sqrt(np.float64(0.625)), "c38": np.sqrt(np.float64(0.375))}


def bits(v):
    return int(np.float64(v).view(np.uint64))


def test_the_reference_constants_are_numpys_square_roots():
    assert {k: bits(v) for k, v in ambi_ref.CONSTANTS.items()} == {k: bits(v) for k, v in WANT.items()}


def test_the_device_constants_are_numpys_square_roots_bit_for_bit():
    src = open(RECEIVE_HIP).read()
    found = {m.group(1).lower(): float.fromhex(m.group(2)) for m in re.finditer(r"constexpr double kAmbi(C\w+) = (0x[0-9a-fA-F.]+p[+-]\d+);", src)}
    assert sorted(found) == sorted(WANT)
    for name, v in WANT.items():
        assert bits(found[name]) == bits(v), name


# ---- known answers
def test_the_zenith_gives_y6_and_y12():
    Y = ambi_ref.harmonics(0.0, 0.0, 1.0)
    assert [float(y) for y in Y] == [0, 0, 1.0, 0, 0, 0, 0, 0, 1.0, 0, 0, 0]


def test_the_x_axis_gives_y8_y15_y6_y13():
    Y = ambi_ref.harmonics(1.0, 0.0, 0.0)
    want = [0.0] * 12
    want[8 - 4], want[15 - 4], want[6 - 4], want[13 - 4] = WANT["c3h"], WANT["c58"], -0.5, -WANT["c38"]
    assert [bits(abs(y)) if y == 0 else bits(y) for y in Y] == [bits(w) for w in want]


def test_order_two_is_the_head_of_order_three():
    rng = np.random.default_rng(3)
    a = rng.normal(size=(3, 100))
    y2, y3 = ambi_ref.harmonics(*a, order=2), ambi_ref.harmonics(*a, order=3)
    assert len(y2) == 5 and len(y3) == 12
    for u, v in zip(y2, y3):
        assert np.array_equal(u.view(np.uint64), v.view(np.uint64))


def test_sn3d_the_squares_of_an_order_sum_to_one():
    """For a unit vector the 2 l + 1 SN3D harmonics of order l have squares that sum to 1.  1e-12: about twenty roundings of 2^-53 on
    terms below 1 (the vector's own normalisation among them)."""
    rng = np.random.default_rng(20261019)
    v = rng.normal(size=(1000, 3))
    v /= np.sqrt((v * v).sum(axis=1))[:, None]
    Y = np.stack(ambi_ref.harmonics(v[:, 0], v[:, 1], v[:, 2]))
    assert np.abs((Y[:5] ** 2).sum(axis=0) - 1.0).max() < 1e-12
    assert np.abs((Y[5:] ** 2).sum(axis=0) - 1.0).max() < 1e-12
    assert np.abs(Y).max() <= 1.0 + 1e-12                                       # the header's headroom rule


# ---- the designed edges are met (tests/ambi_cases.py: edge_case)
def test_the_edge_inputs_reach_the_clamp_and_the_ties():
    from tests.receive_ref import TWO62, magnitude, signed_words
    m = magnitude(np.array([2.0 ** 63, 1e300, 1.0, 3.0]), 0)
    y6 = ambi_ref.harmonics(1.0, 0.0, 0.0)[2]                                   # -0.5
    w = signed_words(m, y6).view(np.int64)
    assert w.tolist() == [-int(TWO62), -int(TWO62), 0, -2]                      # 2^63 * -0.5 = -2^62 exactly; -0.5 and -1.5 are ties: to even
    y8 = ambi_ref.harmonics(1.0, 0.0, 0.0)[4]
    assert signed_words(m[:1], y8).view(np.int64)[0] == int(TWO62)              # 2^63 * 0.866 clamps
    assert signed_words(m[:1], np.float64(np.nan)).view(np.int64)[0] == 0
    a = ac.aimed_rays(17, np.zeros(3))[:, 3:]
    ln = np.sqrt((a * a).sum(axis=1))
    assert set(np.round(ln * ln).astype(int)) == {1, 2, 3}                      # axes and the two kinds of diagonals


# ---- nesting in the reference loop
NEST = [ac.burst_case(257, 3, 3), ac.burst_case(257, 3, 3, mode="rain", seed=9)]


@pytest.mark.parametrize("case", NEST, ids=lambda c: c.name)
def test_channels_nest_in_the_reference(case):
    first = rc.reference(case)                                                  # receive_ref's own directional histogram
    o2 = ac.reference(ac.with_order(case, 2, name=case.name + "-as2"))
    o3 = ac.reference(case)
    assert first["hist"].shape[3] == 4 and o2["hist"].shape[3] == 9 and o3["hist"].shape[3] == 16
    assert np.array_equal(o2["hist"][..., :4], first["hist"]) and np.array_equal(o3["hist"][..., :4], first["hist"])
    assert np.array_equal(o3["hist"][..., :9], o2["hist"])
    assert o3["hist"][..., 4:].any()
    for k in ("det", "state", "rays"):
        assert np.array_equal(o3[k], first[k], equal_nan=True)


def test_the_source_paths_nest_in_the_reference():
    """direct_ref / image_ref / image2_ref deposit through the same widened deposit (direct_ref keeps its results by name: a name each)."""
    import dataclasses
    from tests import direct_ref
    case = next(c for c in direct_ref.cases() if c.name == "K255-dir")
    h1 = direct_ref.reference(case)["hist"]
    h2, h3 = (ambi_ref.run(order, direct_ref.reference, dataclasses.replace(case, name=f"{case.name}-o{order}"))["hist"] for order in (2, 3))
    assert h3.shape[3] == 16 and np.array_equal(h3[..., :4], h1) and np.array_equal(h3[..., :9], h2) and h3[..., 4:].any()


def test_many_lanes_of_a_wave_share_a_bin_in_the_scene_cases():
    """What the aggregated add is there for: in the first wave of the burst, cast 0, most lanes land in one bin of the receiver about the
    source, and several in one bin of the receiver 2 m away."""
    counts = rc.wave_counts(ac.burst_case(4159, 8, 3), 0)
    assert counts[1].max() == 64 and counts[0].max() >= 8, counts.max(axis=1)


# ---- pinned
@pytest.mark.parametrize("case", ac.fixed_cases(), ids=lambda c: c.name)
def test_the_reference_on_the_fixed_cases_is_pinned(case):
    assert ac.digest(ac.reference(case)) == ac.pinned_digests()["fixed/" + case.name]


@pytest.mark.parametrize("seed", ac.SWEEP_SEEDS)
def test_the_reference_on_the_sweep_is_pinned(seed):
    case = ac.sweep_case(seed)
    assert ac.digest(ambi_ref.run(case.order, rc.reference, case)) == ac.pinned_digests()["sweep/%d" % seed]


# ---- the calls' first check (no device: HARE_E_INVALID comes before one is looked for)
@pytest.fixture(scope="module")
def grid():
    m = H.scenes.shoebox(nface=1)
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 2)
    g.set_receivers(np.array([[5.0, 3.5, 2.0]]), np.array([0.5]))
    g.set_source([3.0, 3.0, 1.5])
    return g


BAD_FLAGS = (O2, O3, DIR | O2 | O3, O2 | O3, O3 | capi.RECEIVE_DIFFUSE_RAIN)
A = 0x7000_0000_0000                     # caller buffers are addresses only: the refusal comes before anything is read


def calls(g, flags, n_bins=8):
    lib = capi.lib
    rays = np.zeros((4, 6))
    rays[:, 3] = 1.0
    state, hist, det = np.zeros((2, 4)), np.zeros(1 << 12, np.uint64), np.zeros(2, np.uint64)
    first = np.int64(0)
    return {
        "hare_receive_batch": lambda: lib.hare_receive_batch(g._h, g._kind, 0, 4, capi.ptr(rays), None, None, 1, flags, n_bins, 1.0, 10, None, capi.ptr(state),
                                                             capi.ptr(hist), capi.ptr(det), None),
        "hare_receive_source": lambda: lib.hare_receive_source(g._h, g._kind, 0, 4, int(first), 1, flags, n_bins, 1.0, 10, capi.ptr(state), capi.ptr(hist),
                                                               capi.ptr(det), None),
        "hare_direct_device": lambda: lib.hare_direct_device(g._h, g._kind, 0, 4, flags, n_bins, 1.0, 10, A, A + (1 << 30), A + (2 << 30), None),
        "hare_image_device": lambda: lib.hare_image_device(g._h, g._kind, 0, 4, flags, n_bins, 1.0, 10, 16, A, A + (1 << 30), A + (2 << 30), None),
        "hare_image2_device": lambda: lib.hare_image2_device(g._h, g._kind, 0, 4, flags, n_bins, 1.0, 10, 16, 16, A, A + (1 << 30), A + (2 << 30), None),
    }


@pytest.mark.parametrize("flags", BAD_FLAGS)
@pytest.mark.parametrize("call", ["hare_receive_batch", "hare_receive_source", "hare_direct_device", "hare_image_device", "hare_image2_device"])
def test_an_order_flag_needs_the_directional_flag_and_stands_alone(grid, call, flags):
    assert calls(grid, flags)[call]() == capi.HARE_E_INVALID
    assert "HARE_RECEIVE_ORDER" in capi.last_error() and call in capi.last_error()


@pytest.mark.parametrize("flags", (DIR | O2, DIR | O3))
@pytest.mark.parametrize("call", ["hare_receive_batch", "hare_receive_source"])          # the calls on host buffers: with a device they run
def test_an_order_flag_with_the_directional_flag_passes_the_checks(grid, call, flags):
    rc_ = calls(grid, flags)[call]()
    if rc_ != capi.HARE_OK:                                                     # without a device: every check passed, then no device was found
        assert rc_ == capi.HARE_E_NODEVICE, capi.last_error()


def test_the_histogram_cap_counts_sixteen_channels(grid):
    for flags, C in ((DIR | O3, 16), (DIR | O2, 9)):
        n_bins = (1 << 27) // C + 1                                             # K = 1, B = 1: one entry over the cap at C channels
        for call in ("hare_receive_batch", "hare_receive_source", "hare_direct_device", "hare_image_device", "hare_image2_device"):
            assert calls(grid, flags, n_bins)[call]() == capi.HARE_E_INVALID
            assert "2^27" in capi.last_error()


def test_the_python_binding_shapes_the_histogram_by_order(grid):
    assert grid._receive_shape(0, 8, True, order=2) == (1, 8, 1, 9) and grid._receive_shape(0, 8, True, order=3) == (1, 8, 1, 16)
    assert grid._receive_shape(0, 8, True) == (1, 8, 1, 4) and grid._receive_shape(0, 8, False) == (1, 8, 1)
    with pytest.raises(ValueError):
        grid._receive_shape(0, 8, True, order=4)
    h = np.zeros((1, 8, 1, 16), np.uint64)
    h[..., 5] = np.uint64(2 ** 64 - 3)
    s = H.Voxel_Grid.directional_signed(h)
    assert s.shape == (1, 8, 1, 15) and s.dtype == np.int64 and (s[..., 4] == -3).all()
    with pytest.raises(H.capi.HareError):
        grid.Receive_batch(np.zeros((1, 6)), 1, 8, 1.0, order=2)                # order without directional: the library's refusal


def test_the_reduction_accepts_nine_and_sixteen_channels(grid):
    win, lv = np.array([0, 4], np.int32), np.array([1 << 31], np.uint32)
    for ch, want in ((9, (capi.HARE_OK, capi.HARE_E_NODEVICE)), (16, (capi.HARE_OK, capi.HARE_E_NODEVICE)), (8, (capi.HARE_E_INVALID,)),
                     (12, (capi.HARE_E_INVALID,))):
        hist, sums, cross = np.zeros(2 * 8 * ch, np.uint64), np.zeros(2 * 4, np.uint64), np.zeros(2, np.int32)
        got = capi.lib.hare_hist_reduce(grid._h, 2, 8, 1, ch, capi.ptr(hist), None, 1, capi.ptr(win), 1, capi.ptr(lv), capi.ptr(sums), capi.ptr(cross))
        assert got in want, (ch, capi.last_error())
