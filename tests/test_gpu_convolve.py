"""hare_convolve on the MI355X (include/hare_hip.h, "receivers", "Convolution"): on every case of tests/convolve_cases.py the host call
returns what the numpy restatement (tests/convolve_ref.py) computes -- a NaN where the reference has one, the same 64 bits everywhere else;
the device call on torch tensors writes the window and nothing behind it, allocates nothing, frees nothing and waits for nothing; one job
cut into three output windows is byte for byte the one call; and a third-order histogram rendered by hare_hist_render_device and convolved
by hare_convolve_device on the same stream, without leaving the device, is render_ref followed by convolve_ref."""
import numpy as np
import pytest

import hare_amd as H
from tests.convolve_cases import CASES, TILE, inputs, reference
from tests.convolve_ref import convolve_ref
from tests.receive_harness import CALL_COUNTERS, same_bits

pytestmark = pytest.mark.gpu

GUARD = 64                                            # words behind d_y that must stay as they were
POISON = 0x7FF8DEADBEEF0000                           # a NaN pattern no sum produces


@pytest.fixture(scope="module")
def grid():
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.convolve(np.ones((1, 1)), np.ones(1))           # the module is loaded before a test counts calls
    return g


def run_device(g, ir, x, n0, n_out):
    """hare_convolve_device: (y [R, n_out], the GUARD words behind it as uint64, change of CALL_COUNTERS over the call)"""
    import torch
    R, N = ir.shape
    d_ir, d_x = torch.from_numpy(np.array(ir)).to("cuda"), torch.from_numpy(np.array(x)).to("cuda")
    d_y = torch.full((R * n_out + GUARD,), POISON, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    before = [g.get_option(o) for o in CALL_COUNTERS]
    g.convolve_device(R, N, d_ir.data_ptr(), x.shape[0], d_x.data_ptr(), n0, n_out, d_y.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    after = [g.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    out = d_y.cpu().numpy()
    return out[:R * n_out].view(np.float64).reshape(R, n_out), out[R * n_out:].view(np.uint64), [a - b for a, b in zip(after, before)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_every_case_matches_the_reference_bit_for_bit(grid, case):
    ir, x = inputs(case)
    y = grid.convolve(ir, x, case.n0, case.n_out)
    assert same_bits(y, reference(case)) is None, same_bits(y, reference(case))


@pytest.mark.parametrize("case", [c for c in CASES if c.index % 8 == 0 or c.window.startswith("tile")], ids=lambda c: c.id)
def test_the_device_call_writes_the_window_and_nothing_else(grid, case):
    ir, x = inputs(case)
    y, guard, calls = run_device(grid, ir, x, case.n0, case.n_out)
    assert same_bits(y, reference(case)) is None, same_bits(y, reference(case))
    assert (guard == np.uint64(POISON)).all()
    assert calls == [0, 0, 0], calls


def test_three_output_windows_are_the_one_call_byte_for_byte(grid):
    """Cuts inside a tile of the one call and a sample behind a tile edge: every output is its own sum, so where the window starts is not seen"""
    rng = np.random.default_rng(77)
    ir, x = rng.standard_normal((5, 3000)), rng.standard_normal(2500)
    total = 3000 + 2500 - 1
    whole = grid.convolve(ir, x)
    cuts = [0, 777, TILE + 1, total]
    parts = [grid.convolve(ir, x, a, b - a) for a, b in zip(cuts, cuts[1:])]
    assert whole.shape == (5, total) and np.concatenate(parts, axis=1).tobytes() == whole.tobytes()
    assert same_bits(whole, convolve_ref(ir, x)) is None


def test_render_then_convolve_on_one_stream_without_leaving_the_device(grid):
    """A small third-order histogram: hare_hist_render_device writes K x 16 rows of n_bins x M samples, hare_convolve_device reads them as
    its ir behind it on the same stream; only the convolved signal comes down."""
    import torch
    from tests.render_ref import render_ref
    K, n_bins, B, C, M, T, frac_bits, seed, L = 2, 12, 3, 16, 20, 9, 24, 31337, 700
    rng = np.random.default_rng(5)
    W = rng.integers(1, 1 << 40, (K, n_bins, B), dtype=np.uint64)
    hist = np.zeros((K, n_bins, B, C), np.uint64)
    hist[..., 0] = W
    hist[..., 1:] = np.trunc(rng.uniform(-1, 1, (K, n_bins, B, C - 1)) * W[..., None].astype(np.float64)).astype(np.int64).view(np.uint64)
    taps, x = rng.uniform(-1, 1, (B, T)), rng.standard_normal(L)
    R, N = K * C, n_bins * M
    n_out = N + L - 1
    d_hist = torch.from_numpy(hist.view(np.int64)).to("cuda")
    d_taps, d_x = torch.from_numpy(taps).to("cuda"), torch.from_numpy(x).to("cuda")
    d_ir = torch.full((R * N,), POISON, dtype=torch.int64, device="cuda")
    d_y = torch.full((R * n_out,), POISON, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    before = [grid.get_option(o) for o in CALL_COUNTERS]
    grid.hist_render_device(K, n_bins, B, C, d_hist.data_ptr(), frac_bits, M, T, d_taps.data_ptr(), seed, d_ir.data_ptr(), stream=stream)
    grid.convolve_device(R, N, d_ir.data_ptr(), L, d_x.data_ptr(), 0, n_out, d_y.data_ptr(), stream=stream)
    after = [grid.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    assert after == before
    y = d_y.cpu().numpy().view(np.float64).reshape(R, n_out)
    want = convolve_ref(render_ref(hist, taps, M, frac_bits, seed), x)
    assert want.shape == y.shape and np.isfinite(want).all() and want.any()
    assert same_bits(y, want) is None, same_bits(y, want)
