"""hare_hist_reduce on the MI355X (include/hare_hip.h, "receivers", "Reduction"): the device call on torch tensors and the host call
return, byte for byte, what the integer restatement (tests/reduce_ref.py) computes -- over a pairwise cover of the shapes at the
kernel's tile, wave and carry edges, every word class with every kind of weights, histograms of nine and sixteen channels (the higher
orders' strides), the window and level sets of tests/reduce_cases.py.  The device call allocates nothing, frees nothing and waits for nothing, and two runs give the same bytes."""
import numpy as np
import pytest

import hare_amd as H
from tests.receive_harness import CALL_COUNTERS, same_bits
from tests.reduce_cases import CLASSES, COVER, STRIDES, inputs, reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def grid():
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.hist_reduce(np.ones((1, 1, 1), np.uint64), windows=[(0, 1)])          # the module is loaded before a test counts calls
    return g


def run_device(g, case, poison=0):
    """hare_hist_reduce_device on the case: (sums, cross, change of CALL_COUNTERS over the call).  The outputs start out as `poison`."""
    import torch
    hist, weight = inputs(case)
    K, B, n_win, n_lev = case.K, case.B, len(case.windows), len(case.levels)
    d_hist = torch.from_numpy(hist.view(np.int64)).to("cuda")
    d_weight = None if weight is None else torch.from_numpy(weight.view(np.int32)).to("cuda")
    d_sums = torch.full((max(1, K * B * n_win * 4),), poison, dtype=torch.int64, device="cuda")
    d_cross = torch.full((max(1, K * B * n_lev),), poison, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    before = [g.get_option(o) for o in CALL_COUNTERS]
    g.hist_reduce_device(K, case.n_bins, B, case.channels, d_hist.data_ptr(), d_sums.data_ptr() if n_win else 0,
                         d_cross.data_ptr() if n_lev else 0, windows=case.windows, levels=case.levels,
                         d_weight=0 if d_weight is None else d_weight.data_ptr())
    after = [g.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    sums = d_sums.cpu().numpy().view(np.uint64)[:K * B * n_win * 4].reshape(K, B, n_win, 4)
    cross = d_cross.cpu().numpy()[:K * B * n_lev].reshape(K, B, n_lev)
    return sums, cross, [a - b for a, b in zip(after, before)]


def check(g, case):
    want_sums, want_cross = reference(case)
    sums, cross, calls = run_device(g, case, poison=-1)
    assert same_bits(sums, want_sums) is None, "device sums: " + same_bits(sums, want_sums)
    assert same_bits(cross, want_cross) is None, "device crossings: " + same_bits(cross, want_cross)
    assert calls == [0, 0, 0], calls
    hist, weight = inputs(case)
    sums, cross = g.hist_reduce(hist, case.windows, case.levels, weight)
    assert same_bits(sums, want_sums) is None, "host sums: " + same_bits(sums, want_sums)
    assert same_bits(cross, want_cross) is None, "host crossings: " + same_bits(cross, want_cross)


@pytest.mark.parametrize("case", COVER, ids=lambda c: c.id)
def test_shapes_at_the_tile_wave_and_carry_edges(grid, case):
    check(grid, case)


@pytest.mark.parametrize("case", CLASSES, ids=lambda c: c.id)
def test_every_word_class_with_every_weight(grid, case):
    check(grid, case)


@pytest.mark.parametrize("case", STRIDES, ids=lambda c: c.id)
def test_channel_0_is_read_at_the_strides_of_nine_and_sixteen_channels(grid, case):
    check(grid, case)


def test_two_runs_give_identical_bytes_whatever_the_outputs_held(grid):
    case = COVER[39]                                                        # n_bins 4097, full-range words
    a, b = run_device(grid, case, poison=0), run_device(grid, case, poison=0x5A5A5A5A)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[2] == [0, 0, 0] and b[2] == [0, 0, 0]
