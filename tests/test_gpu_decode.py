"""hare_decode on the MI355X (include/hare_hip.h, "receivers", "Decoding"): on every case of tests/decode_cases.py the host call returns what
the numpy restatement (tests/decode_ref.py) computes -- a NaN where the reference has one, the same 64 bits everywhere else; the device
call on torch tensors writes the window and nothing behind it, allocates nothing, frees nothing and waits for nothing; one job cut into
three output windows, and cut per output o, and per receiver k, is byte for byte the one call; with C = O = 1 the call is hare_convolve on
the device, byte for byte; and a third-order histogram rendered by hare_hist_render_device, decoded to two outputs by hare_decode_device
and convolved with a signal by hare_convolve_device on the same stream, without leaving the device, is render_ref, then decode_ref, then
convolve_ref."""
import numpy as np
import pytest

import hare_amd as H
from tests.convolve_ref import convolve_ref
from tests.decode_cases import CASES, TILE, inputs, reference
from tests.decode_ref import decode_ref
from tests.receive_harness import CALL_COUNTERS, same_bits

pytestmark = pytest.mark.gpu

GUARD = 64                                            # words behind d_y that must stay as they were
POISON = 0x7FF8DEADBEEF0000                           # a NaN pattern no sum produces


@pytest.fixture(scope="module")
def grid():
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.decode(np.ones((1, 1, 1)), np.ones((1, 1, 1)))          # the module is loaded before a test counts calls
    return g


def run_device(g, x, h, n0, n_out):
    """hare_decode_device: (y [K, O, n_out], the GUARD words behind it as uint64, change of CALL_COUNTERS over the call)"""
    import torch
    (K, C, N), (O, _, T) = x.shape, h.shape
    d_x, d_h = torch.from_numpy(np.array(x)).to("cuda"), torch.from_numpy(np.array(h)).to("cuda")
    d_y = torch.full((K * O * n_out + GUARD,), POISON, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    before = [g.get_option(o) for o in CALL_COUNTERS]
    g.decode_device(K, C, N, d_x.data_ptr(), O, T, d_h.data_ptr(), n0, n_out, d_y.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    after = [g.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    out = d_y.cpu().numpy()
    return out[:K * O * n_out].view(np.float64).reshape(K, O, n_out), out[K * O * n_out:].view(np.uint64), [a - b for a, b in zip(after, before)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_every_case_matches_the_reference_bit_for_bit(grid, case):
    x, h = inputs(case)
    y = grid.decode(x, h, case.n0, case.n_out)
    assert y.shape == reference(case).shape
    assert same_bits(y, reference(case)) is None, same_bits(y, reference(case))


@pytest.mark.parametrize("case", [c for c in CASES if c.index % 5 == 0 or c.window.startswith("tile")], ids=lambda c: c.id)
def test_the_device_call_writes_the_window_and_nothing_else(grid, case):
    x, h = inputs(case)
    y, guard, calls = run_device(grid, x, h, case.n0, case.n_out)
    assert same_bits(y, reference(case)) is None, same_bits(y, reference(case))
    assert (guard == np.uint64(POISON)).all()
    assert calls == [0, 0, 0], calls


def test_a_job_cut_over_windows_outputs_or_receivers_is_the_one_call_byte_for_byte(grid):
    """Cuts inside a tile of the one call and a sample behind a tile edge; then one call per output o (a row of h) and one per receiver k
    (a row of in): every output is its own sum, so where the window starts, and what else the call computes, is not seen"""
    rng = np.random.default_rng(77)
    K, C, O, N, T = 2, 9, 3, 3000, 300
    x, h = rng.standard_normal((K, C, N)), rng.standard_normal((O, C, T))
    total = N + T - 1
    whole = grid.decode(x, h)
    assert whole.shape == (K, O, total) and same_bits(whole, decode_ref(x, h)) is None
    cuts = [0, 777, TILE + 1, total]
    parts = [grid.decode(x, h, a, b - a) for a, b in zip(cuts, cuts[1:])]
    assert np.concatenate(parts, axis=2).tobytes() == whole.tobytes()
    per_o = [grid.decode(x, h[o:o + 1]) for o in range(O)]
    assert np.concatenate(per_o, axis=1).tobytes() == whole.tobytes()
    per_k = [grid.decode(x[k:k + 1], h) for k in range(K)]
    assert np.concatenate(per_k, axis=0).tobytes() == whole.tobytes()


@pytest.mark.parametrize("N,T", ((3000, 300), (300, 3000), (700, 31), (1, 1)))
def test_one_channel_and_one_output_is_hare_convolve_byte_for_byte(grid, N, T):
    """hare_convolve with ir = h (R = 1, its N this T) and x = in[k], receiver by receiver, both on the device"""
    rng = np.random.default_rng(N + T)
    K = 3
    x, h = rng.standard_normal((K, 1, N)), rng.standard_normal((1, 1, T))
    x[1, 0, N // 2], h[0, 0, T // 3] = 1e300, -0.0          # no NaN: its payload alone is not defined
    for n0, n_out in ((0, N + T - 1), ((N + T - 1) // 3, (N + T) // 2)):
        y = grid.decode(x, h, n0, n_out)
        for k in range(K):
            assert y[k].tobytes() == grid.convolve(h[0], x[k, 0], n0, n_out).tobytes(), (k, n0)


def test_render_then_decode_then_convolve_on_one_stream_without_leaving_the_device(grid):
    """A small third-order histogram: hare_hist_render_device writes K x 16 rows of n_bins x M samples, hare_decode_device reads them as
    its `in` behind it on the same stream and writes K x 2 rows, hare_convolve_device reads those as its ir; only the sound comes down."""
    import torch
    from tests.render_ref import render_ref
    K, n_bins, B, C, M, Tr, frac_bits, seed, O, T, L = 2, 12, 3, 16, 20, 9, 24, 31337, 2, 40, 700
    rng = np.random.default_rng(6)
    W = rng.integers(1, 1 << 40, (K, n_bins, B), dtype=np.uint64)
    hist = np.zeros((K, n_bins, B, C), np.uint64)
    hist[..., 0] = W
    hist[..., 1:] = np.trunc(rng.uniform(-1, 1, (K, n_bins, B, C - 1)) * W[..., None].astype(np.float64)).astype(np.int64).view(np.uint64)
    taps, h, x = rng.uniform(-1, 1, (B, Tr)), rng.standard_normal((O, C, T)), rng.standard_normal(L)
    N = n_bins * M
    Nd = N + T - 1                                    # the decoded rows, whole
    n_out = Nd + L - 1
    d_hist = torch.from_numpy(hist.view(np.int64)).to("cuda")
    d_taps, d_h, d_x = torch.from_numpy(taps).to("cuda"), torch.from_numpy(h).to("cuda"), torch.from_numpy(x).to("cuda")
    d_ir = torch.full((K * C * N,), POISON, dtype=torch.int64, device="cuda")
    d_dec = torch.full((K * O * Nd,), POISON, dtype=torch.int64, device="cuda")
    d_y = torch.full((K * O * n_out,), POISON, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    before = [grid.get_option(o) for o in CALL_COUNTERS]
    grid.hist_render_device(K, n_bins, B, C, d_hist.data_ptr(), frac_bits, M, Tr, d_taps.data_ptr(), seed, d_ir.data_ptr(), stream=stream)
    grid.decode_device(K, C, N, d_ir.data_ptr(), O, T, d_h.data_ptr(), 0, Nd, d_dec.data_ptr(), stream=stream)
    grid.convolve_device(K * O, Nd, d_dec.data_ptr(), L, d_x.data_ptr(), 0, n_out, d_y.data_ptr(), stream=stream)
    after = [grid.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    assert after == before
    y = d_y.cpu().numpy().view(np.float64).reshape(K * O, n_out)
    rendered = render_ref(hist, taps, M, frac_bits, seed)
    want = convolve_ref(decode_ref(rendered.reshape(K, C, N), h), x)
    assert want.shape == y.shape and np.isfinite(want).all() and want.any()
    assert same_bits(y, want) is None, same_bits(y, want)
