"""hare_hist_project_channels on the MI355X (include/hare_hip.h, "receivers", "Directional projection"): the host call and, on a fifth
of the cases, the device call on torch tensors return, word for word, what the integer restatement (tests/project_channels_ref.py)
computes -- over the fixed cases of tests/project_channels_cases.py (a pairwise cover of every (B, channels) with the bin counts at the
kernel's tile edges and the vector counts around its sweep group, every word class with every kind of weights, the "negative weighted"
cases, the idle-thread shape) and a seeded sweep of 50.  The device call writes every output word and none behind them, allocates nothing,
frees nothing and waits for nothing.  Without weights the projections of two shards sum to the projection of the summed histogram; the
column ch = 0 is hare_hist_project's on the device; and a histogram the receive loop accumulated at ambisonic order 2 goes through."""
import numpy as np
import pytest

import hare_amd as H
from tests.project_channels_cases import CLASSES, COVER, IDLE, NEGATIVE_WEIGHTED, Case, inputs, reference, sweep_case
from tests.project_channels_ref import project_channels_ref, to_int
from tests.receive_harness import CALL_COUNTERS, same_bits

pytestmark = pytest.mark.gpu

GUARD = 64                                   # words behind d_proj that the device call must leave alone
POISON = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def grid():
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.hist_project_channels(np.ones((1, 1, 1), np.uint64), np.ones((1, 1), np.int32))      # the module is loaded before a test counts calls
    return g


def run_device(g, case):
    """hare_hist_project_channels_device on the case: (proj, the guard words behind it, change of CALL_COUNTERS over the call)."""
    import torch
    hist, coef, weight = inputs(case)
    K, B, J, C = case.K, case.B, case.J, case.channels
    n = K * B * J * C * 2
    d_hist = torch.from_numpy(hist.view(np.int64)).to("cuda")
    d_coef = torch.from_numpy(coef).to("cuda")
    d_weight = None if weight is None else torch.from_numpy(weight.view(np.int32)).to("cuda")
    d_proj = torch.full((n + GUARD,), POISON, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    before = [g.get_option(o) for o in CALL_COUNTERS]
    g.hist_project_channels_device(K, case.n_bins, B, C, d_hist.data_ptr(), J, d_coef.data_ptr(), d_proj.data_ptr(),
                                   d_weight=0 if d_weight is None else d_weight.data_ptr())
    after = [g.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    out = d_proj.cpu().numpy().view(np.uint64)
    return out[:n].reshape(K, B, J, C, 2), out[n:], [a - b for a, b in zip(after, before)]


def check(g, case):
    want = reference(case)
    if case.device:
        proj, guard, calls = run_device(g, case)
        assert same_bits(proj, want) is None, "device: " + same_bits(proj, want)
        assert (guard == np.uint64(POISON)).all() and calls == [0, 0, 0], (guard, calls)
    else:
        hist, coef, weight = inputs(case)
        proj = g.hist_project_channels(hist, coef, weight)
        assert same_bits(proj, want) is None, "host: " + same_bits(proj, want)


@pytest.mark.parametrize("case", COVER, ids=lambda c: c.id)
def test_every_band_and_channel_count_at_the_tile_and_sweep_edges(grid, case):
    check(grid, case)


@pytest.mark.parametrize("case", CLASSES + NEGATIVE_WEIGHTED + IDLE, ids=lambda c: c.id)
def test_every_word_class_with_every_weight_negative_weighted_words_and_idle_threads(grid, case):
    check(grid, case)


@pytest.mark.parametrize("seed", range(50))
def test_seeded_sweep(grid, seed):
    check(grid, sweep_case(seed))


def test_unweighted_projections_of_two_shards_sum_to_the_projection_of_the_sum(grid):
    """Two histograms as two shards of the rays would leave them; their sum as integers (no word overflows: the halves are below 2^62 in
    magnitude)."""
    rng = np.random.default_rng(77)
    K, n, B, C, J = 3, 257, 5, 9, 9
    shards = []
    for _ in range(2):
        h = np.zeros((K, n, B, C), np.uint64)
        h[..., 0] = rng.integers(0, 1 << 62, (K, n, B), dtype=np.uint64)
        h[..., 1:].view(np.int64)[...] = rng.integers(-(1 << 62), 1 << 62, (K, n, B, C - 1), dtype=np.int64)
        shards.append(h)
    with np.errstate(over="ignore"):
        whole = shards[0] + shards[1]                                        # two's complement: the signed words add as int64
    coef = rng.integers(-(1 << 31), 1 << 31, (J, n), dtype=np.int64).astype(np.int32)
    a, b, s = (grid.hist_project_channels(h, coef, as_int=True) for h in (*shards, whole))
    assert (a + b == s).all() and (s == to_int(project_channels_ref(whole, coef))).all()


@pytest.mark.parametrize("shape", ((1, 3, 4, 1, 1), (3, 33, 4, 8, 8), (1, 257, 9, 7, 9), (3, 1000, 16, 8, 17), (1, 256, 16, 3, 32)),
                         ids=lambda s: "K%d-n%d-c%d-B%d-J%d" % s)
def test_column_zero_is_the_projection_on_the_device(grid, shape):
    K, n, C, B, J = shape
    case = Case(7000 + n, n, B, C, K, J, word="full", coef=6, weight="random" if n & 1 else "none")
    hist, coef, weight = inputs(case)
    got = grid.hist_project_channels(hist, coef, weight)
    assert got[:, :, :, 0].tobytes() == grid.hist_project(hist, coef, weight).tobytes()
    assert same_bits(got, reference(case)) is None


def test_a_second_order_histogram_of_the_receive_loop_goes_through():
    """A shoebox, a point source, four receivers, 65 536 rays at ambisonic order 2: the histogram of hare_receive_source, projected onto
    four windows, equals the restatement on the same histogram bit for bit, with and without air absorption."""
    from hare_amd import spatial
    K, n_bins, B, bin_len = 4, 64, 2, 1.0
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.set_absorption(np.tile([0.1, 0.3], (m.verts.shape[0], 1)))
    g.set_source([2.0, 3.5, 1.7])
    g.set_receivers([[6.0, 3.0, 1.2], [8.0, 5.0, 1.5], [3.0, 1.5, 2.0], [5.0, 5.5, 1.0]], [0.5] * K)
    hist = g.Receive_source(65536, 12, n_bins, bin_len, frac_bits=30, directional=True, order=2)[0]
    assert hist.shape == (K, n_bins, B, 9) and hist[..., 0].any(axis=(1, 2)).all()
    assert (hist[..., 1:].view(np.int64) < 0).any() and hist[..., 4:].any()
    table = spatial.window_vectors(n_bins, bin_len, 343.0, [(0.0, 0.005), (0.005, 0.08), (0.0, 0.08), (0.08, None)])
    for weight in (None, H.air_weights([0.01, 0.05], bin_len, n_bins)):
        proj = g.hist_project_channels(hist, table, weight)
        assert same_bits(proj, project_channels_ref(hist, table, weight)) is None
    lf = spatial.lateral_fraction(proj, [0.0, 1.0, 0.0], early=1, total=2)
    assert lf.shape == (K, B) and np.isfinite(lf).all() and (lf > 0).all() and (lf < 1).all(), lf
