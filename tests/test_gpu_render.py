"""hare_hist_render on the MI355X (include/hare_hip.h, "receivers", "Rendering"): the device call on torch tensors and the host call return,
byte for byte, what the numpy restatement (tests/render_ref.py) computes -- on every fixed case of tests/render_cases.py (the tile, halo
and mask-word edges, every word class, every kind of taps) and on every seed of its sweep.  The output starts out as poison, the device
call allocates nothing, frees nothing and waits for nothing, and two runs give the same bytes."""
import numpy as np
import pytest

import hare_amd as H
from tests.receive_harness import CALL_COUNTERS, same_bits
from tests.render_cases import BY_CLASS, FIXED, SWEEP, inputs, reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def grid():
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.hist_render(np.ones((1, 1, 1), np.uint64), np.ones((1, 1)), 1, 0)     # the module is loaded before a test counts calls
    return g


def run_device(g, case, poison):
    """hare_hist_render_device on the case: (out [K, channels, N], change of CALL_COUNTERS over the call).  The output starts out as the
    64-bit pattern `poison`."""
    import torch
    hist, weight, taps = inputs(case)
    d_hist = torch.from_numpy(hist.view(np.int64)).to("cuda")
    d_weight = None if weight is None else torch.from_numpy(weight.view(np.int32)).to("cuda")
    d_taps = torch.from_numpy(taps).to("cuda")
    d_out = torch.full((case.K * case.channels * case.N,), poison, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    before = [g.get_option(o) for o in CALL_COUNTERS]
    g.hist_render_device(case.K, case.n_bins, case.B, case.channels, d_hist.data_ptr(), case.frac_bits, case.M, case.T, d_taps.data_ptr(),
                         case.seed, d_out.data_ptr(), d_weight=0 if d_weight is None else d_weight.data_ptr())
    after = [g.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.float64).reshape(case.K, case.channels, case.N)
    return out, [a - b for a, b in zip(after, before)]


def check(g, case):
    want = reference(case)
    out, calls = run_device(g, case, poison=0x7FF8DEADBEEF0000)             # a NaN: a word left unwritten cannot pass for a result
    assert same_bits(out, want) is None, "device call: " + same_bits(out, want)
    assert calls == [0, 0, 0], calls
    hist, weight, taps = inputs(case)
    out = g.hist_render(hist, taps, case.M, case.frac_bits, case.seed, weight)
    assert same_bits(out, want) is None, "host call: " + same_bits(out, want)


@pytest.mark.parametrize("case", FIXED, ids=lambda c: c.id)
def test_fixed_cases_match_the_reference_bit_for_bit(grid, case):
    check(grid, case)


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: c.id)
def test_the_seeded_sweep_matches_the_reference_bit_for_bit(grid, case):
    check(grid, case)


def test_two_runs_give_identical_bytes_whatever_the_output_held(grid):
    case = BY_CLASS["several tiles"]
    a, b = run_device(grid, case, poison=0), run_device(grid, case, poison=0x5A5A5A5A5A5A5A5A)
    assert a[0].tobytes() == b[0].tobytes()
    assert a[1] == [0, 0, 0] and b[1] == [0, 0, 0]
