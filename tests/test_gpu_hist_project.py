"""hare_hist_project on the MI355X (include/hare_hip.h, "receivers", "Projection"): the device call on torch tensors and the host call
return, byte for byte, what the integer restatement (tests/project_ref.py) computes -- over the fixed cases of tests/project_cases.py (a
pairwise cover of the shapes at the kernel's tile, wave and sweep edges, every word class with every kind of weights and every
coefficient class, nine and sixteen channels with garbage beside W, the vector counts around the sweep group) and a seeded sweep of 50.
The device call writes every output word (the buffer starts out as 0xFF bytes), allocates nothing, frees nothing and waits for nothing,
and two runs give the same bytes."""
import numpy as np
import pytest

import hare_amd as H
from tests.project_cases import CLASSES, COVER, EXTREMES, GROUPS, HIGHER, inputs, reference, sweep_case
from tests.receive_harness import CALL_COUNTERS, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def grid():
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.hist_project(np.ones((1, 1, 1), np.uint64), np.ones((1, 1), np.int32))          # the module is loaded before a test counts calls
    return g


def run_device(g, case, poison=-1):
    """hare_hist_project_device on the case: (proj, change of CALL_COUNTERS over the call).  The output starts out as `poison`."""
    import torch
    hist, coef, weight = inputs(case)
    K, B, J = case.K, case.B, case.J
    d_hist = torch.from_numpy(hist.view(np.int64)).to("cuda")
    d_coef = torch.from_numpy(coef).to("cuda")
    d_weight = None if weight is None else torch.from_numpy(weight.view(np.int32)).to("cuda")
    d_proj = torch.full((K * B * J * 2,), poison, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    before = [g.get_option(o) for o in CALL_COUNTERS]
    g.hist_project_device(K, case.n_bins, B, case.channels, d_hist.data_ptr(), J, d_coef.data_ptr(), d_proj.data_ptr(),
                          d_weight=0 if d_weight is None else d_weight.data_ptr())
    after = [g.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    return d_proj.cpu().numpy().view(np.uint64).reshape(K, B, J, 2), [a - b for a, b in zip(after, before)]


def check(g, case):
    want = reference(case)
    proj, calls = run_device(g, case)                                        # every byte 0xFF before the call
    assert same_bits(proj, want) is None, "device: " + same_bits(proj, want)
    assert calls == [0, 0, 0], calls
    hist, coef, weight = inputs(case)
    proj = g.hist_project(hist, coef, weight)
    assert same_bits(proj, want) is None, "host: " + same_bits(proj, want)


@pytest.mark.parametrize("case", COVER, ids=lambda c: c.id)
def test_shapes_at_the_tile_wave_and_sweep_edges(grid, case):
    check(grid, case)


@pytest.mark.parametrize("case", CLASSES + EXTREMES, ids=lambda c: c.id)
def test_every_word_and_coefficient_class_with_every_weight(grid, case):
    check(grid, case)


@pytest.mark.parametrize("case", GROUPS, ids=lambda c: c.id)
def test_vector_counts_around_the_sweep_group(grid, case):
    check(grid, case)


@pytest.mark.parametrize("case", HIGHER, ids=lambda c: c.id)
def test_nine_and_sixteen_channels_read_w_alone(grid, case):
    check(grid, case)
    hist, coef, weight = inputs(case)                                        # the result is that of the W words alone ...
    alone = grid.hist_project(np.ascontiguousarray(hist[..., 0]), coef, weight)
    other = hist.copy()
    other[..., 1:] = ~other[..., 1:]                                         # ... whatever the other channels hold
    assert grid.hist_project(hist, coef, weight).tobytes() == alone.tobytes() == grid.hist_project(other, coef, weight).tobytes()


@pytest.mark.parametrize("seed", range(50))
def test_seeded_sweep(grid, seed):
    check(grid, sweep_case(seed))


def test_two_runs_give_identical_bytes_whatever_the_output_held(grid):
    for case in (GROUPS[-1], CLASSES[15]):                                   # 32 vectors, B = 8; B = 3 (idle threads), random weights, two sweeps
        assert case.word == "full" and (case.J == 32 or (case.B == 3 and case.weight_kind == "random"))
        a, b = run_device(grid, case, poison=0), run_device(grid, case, poison=0x5A5A5A5A)
        assert a[0].tobytes() == b[0].tobytes() == reference(case).tobytes()
        assert a[1] == [0, 0, 0] and b[1] == [0, 0, 0]
