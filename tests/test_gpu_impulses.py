"""hare_hist_impulses and hare_source_paths on the MI355X (include/hare_hip.h, "receivers", "Impulses"): on every case of
tests/impulse_cases.py the call returns what the numpy restatement (tests/impulse_ref.py) computes -- a NaN where the reference has one,
the same 64 bits everywhere else, the stride gaps and an `out` pre-filled with a sentinel included; the device call on torch tensors
writes its window and nothing else, allocates nothing, frees nothing and waits for nothing, twice the same bytes; a job cut into three
windows is the one call byte for byte; hare_hist_render_device then hare_hist_impulses_device with add == 1 on one stream is render_ref
+ impulse_ref; hare_source_paths at a bin of one sample is the sum of tests/direct_ref.py, image_ref.py and image2_ref.py word for word,
with every flag alone too; and deposits, impulses and hare_decode_device chained on one stream without leaving the device are the
references chained."""
import numpy as np
import pytest

import hare_amd as H
from tests import path_cases as pc
from tests.decode_ref import decode_ref
from tests.impulse_cases import CASES, SENTINEL, TILE, inputs, reference
from tests.impulse_ref import impulse_ref
from tests.path_harness import library_partition
from tests.receive_harness import CALL_COUNTERS, same_bits

pytestmark = pytest.mark.gpu

GUARD = 64                                            # words behind d_out that must stay as they were
FS, C_SOUND = 48000, 343.0


@pytest.fixture(scope="module")
def grid():
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.hist_impulses(np.ones((1, 1, 1), np.uint64), np.ones((1, 1)), 0)          # the module is loaded before a test counts calls
    return g


def run_host(g, case):
    x = inputs(case)
    out = np.array(x["out0"])
    w = None if x["weight"] is None else np.ascontiguousarray(x["weight"])
    rc = H.capi.lib.hare_hist_impulses(g._h, case.K, case.n_bins, case.B, case.C, x["hist"].ctypes.data, None if w is None else w.ctypes.data, case.frac_bits,
                                       case.T, x["taps"].ctypes.data, case.n0, case.n_out, case.stride, 0 if case.add is None else 1, out.ctypes.data)
    assert rc == 0, H.capi.last_error()
    return out


def run_device(g, case):
    """hare_hist_impulses_device: (out [K, C, stride], the GUARD words behind it as uint64, change of CALL_COUNTERS over the call)"""
    import torch
    x = inputs(case)
    words = case.K * case.C * case.stride
    d_hist = torch.from_numpy(np.array(x["hist"]).view(np.int64)).to("cuda")
    d_taps = torch.from_numpy(np.array(x["taps"])).to("cuda")
    d_w = None if x["weight"] is None else torch.from_numpy(np.array(x["weight"]).view(np.int32)).to("cuda")
    host = np.concatenate([x["out0"].reshape(-1).view(np.uint64), np.full(GUARD, SENTINEL, np.uint64)])
    d_out = torch.from_numpy(host.view(np.int64)).to("cuda")
    torch.cuda.synchronize()
    before = [g.get_option(o) for o in CALL_COUNTERS]
    g.hist_impulses_device(case.K, case.n_bins, case.B, case.C, d_hist.data_ptr(), case.frac_bits, case.T, d_taps.data_ptr(), case.n0, case.n_out,
                           case.stride, 0 if case.add is None else 1, d_out.data_ptr(), d_weight=0 if d_w is None else d_w.data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream)
    after = [g.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    return out[:words].view(np.float64).reshape(case.K, case.C, case.stride), out[words:].view(np.uint64), [a - b for a, b in zip(after, before)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_every_case_matches_the_reference_bit_for_bit(grid, case):
    """the host call; a case with a tap that is not finite goes through the device call, which does not refuse it"""
    y = run_device(grid, case)[0] if case.device_only else run_host(grid, case)
    assert same_bits(y, reference(case)) is None, same_bits(y, reference(case))


@pytest.mark.parametrize("case", [c for c in CASES if c.index % 5 == 0 or c.device_only], ids=lambda c: c.id)
def test_the_device_call_writes_the_window_and_nothing_else(grid, case):
    y, guard, calls = run_device(grid, case)
    assert same_bits(y, reference(case)) is None, same_bits(y, reference(case))          # the stride gaps are part of the comparison
    assert (guard == np.uint64(SENTINEL)).all()
    assert calls == [0, 0, 0], calls
    again = run_device(grid, case)[0]
    assert again.tobytes() == y.tobytes() or np.isnan(y).any()
    assert same_bits(again, y) is None


def test_a_job_cut_over_windows_or_receivers_is_the_one_call_byte_for_byte(grid):
    rng = np.random.default_rng(41)
    K, nb, B, C, T = 3, 700, 3, 9, 65
    W = np.where(rng.random((K, nb, B)) < 0.1, rng.integers(1, 1 << 40, (K, nb, B), dtype=np.uint64), np.uint64(0))
    hist = np.zeros((K, nb, B, C), np.uint64)
    hist[..., 0] = W
    hist[..., 1:] = np.trunc(rng.uniform(-1, 1, (K, nb, B, C - 1)) * W[..., None].astype(np.float64)).astype(np.int64).view(np.uint64)
    taps = rng.standard_normal((B, T))
    total = nb + T - 1
    whole = grid.hist_impulses(hist, taps, 24)
    assert whole.shape == (K, C, total) and same_bits(whole, impulse_ref(hist, taps, 24)) is None and whole.any()
    cuts = [0, 100, TILE + 1, total]
    parts = [grid.hist_impulses(hist, taps, 24, a, b - a) for a, b in zip(cuts, cuts[1:])]
    assert np.concatenate(parts, axis=2).tobytes() == whole.tobytes()
    per_k = [grid.hist_impulses(hist[k:k + 1], taps, 24) for k in range(K)]
    assert np.concatenate(per_k, axis=0).tobytes() == whole.tobytes()


def test_render_then_impulses_added_on_one_stream(grid):
    """the hybrid response: the noise rows of hare_hist_render_device, then the impulses of another histogram of the same receivers added
    onto their first n_out samples by hare_hist_impulses_device, out_stride the rendered rows' length"""
    import torch
    from tests.render_ref import render_ref
    rng = np.random.default_rng(8)
    K, B, C, M, Tr, fb, seed = 2, 3, 4, 20, 9, 24, 99
    nb_late, nb, T = 30, 400, 33                       # the rendered rows: 600 samples; the impulses' window: the first 432 of them
    late = np.zeros((K, nb_late, B, C), np.uint64)
    late[..., 0] = rng.integers(1, 1 << 40, (K, nb_late, B), dtype=np.uint64)
    late[..., 1:] = np.trunc(rng.uniform(-1, 1, (K, nb_late, B, C - 1)) * late[..., :1].astype(np.float64)).astype(np.int64).view(np.uint64)
    W = np.where(rng.random((K, nb, B)) < 0.05, rng.integers(1, 1 << 40, (K, nb, B), dtype=np.uint64), np.uint64(0))
    early = np.zeros((K, nb, B, C), np.uint64)
    early[..., 0] = W
    early[..., 1:] = np.trunc(rng.uniform(-1, 1, (K, nb, B, C - 1)) * W[..., None].astype(np.float64)).astype(np.int64).view(np.uint64)
    rtaps, taps = rng.uniform(-1, 1, (B, Tr)), rng.standard_normal((B, T))
    N, n_out = nb_late * M, nb + T - 1
    assert n_out < N
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    d_late, d_early, d_rtaps, d_taps = dev(late.view(np.int64)), dev(early.view(np.int64)), dev(rtaps), dev(taps)
    d_out = torch.full((K * C * N,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    before = [grid.get_option(o) for o in CALL_COUNTERS]
    grid.hist_render_device(K, nb_late, B, C, d_late.data_ptr(), fb, M, Tr, d_rtaps.data_ptr(), seed, d_out.data_ptr(), stream=stream)
    grid.hist_impulses_device(K, nb, B, C, d_early.data_ptr(), fb, T, d_taps.data_ptr(), 0, n_out, N, 1, d_out.data_ptr(), stream=stream)
    after = [grid.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    assert after == before
    y = d_out.cpu().numpy().view(np.float64).reshape(K, C, N)
    want = impulse_ref(early, taps, fb, 0, n_out, out=render_ref(late, rtaps, M, fb, seed), add=1)
    assert np.isfinite(want).all() and (want[..., :n_out] != render_ref(late, rtaps, M, fb, seed)[..., :n_out]).any()
    assert same_bits(y, want) is None, same_bits(y, want)


# ---- hare_source_paths
def shoebox_case(order):
    return pc.axis_box(f"impulses-box-o{order}", max(order, 1)).without(directional=order > 0, n_bins=2048, bin_len=C_SOUND / FS)


def oblique_case(order):
    m, size, pos, placed, rng = pc._box(2, 95, extra=8)
    c, r = pc.receivers_in(rng, m, size, 6, placed)
    return pc.make(f"impulses-oblique-o{order}", m, pc.V8, pos, c, r, B=3, R=4, tables="alpha+sigma", n_bins=2048, bin_len=C_SOUND / FS,
                   directional=order > 0, order=max(order, 1), scene="box2+soup")


FLAGS = dict(direct=dict(direct=True, image=False, image2=False), image=dict(direct=False, image=True, image2=False))


def summed(want, orders):
    with np.errstate(over="ignore"):
        return sum(want[o]["hist"] for o in orders), sum(want[o]["det"] for o in orders)


@pytest.mark.parametrize("room", (shoebox_case, oblique_case), ids=("shoebox", "oblique"))
@pytest.mark.parametrize("order", (0, 3))
def test_source_paths_is_the_sum_of_the_three_references(room, order):
    case = room(order)
    want = pc.reference(case)
    g, _ = library_partition(case)
    kw = dict(frac_bits=case.frac_bits, directional=case.directional, order=case.order)
    hist, det = g.Source_paths(case.n_weight, case.n_bins, case.bin_len, **kw)
    wh, wd = summed(want, pc.ORDERS)
    assert hist.shape == case.shape and wh.any()
    assert np.array_equal(hist, wh) and np.array_equal(det, wd)
    for name, flags in FLAGS.items():                  # each flag alone (HARE_RECEIVE_IMAGE2 stands on _IMAGE: the pair, less the first order)
        h1, d1 = g.Source_paths(case.n_weight, case.n_bins, case.bin_len, **kw, **flags)
        assert np.array_equal(h1, want[name]["hist"]) and np.array_equal(d1, want[name]["det"]), name
    h2, d2 = g.Source_paths(case.n_weight, case.n_bins, case.bin_len, **kw, direct=False)
    wh2, wd2 = summed(want, ("image", "image2"))
    assert np.array_equal(h2, wh2) and np.array_equal(d2, wd2)
    with np.errstate(over="ignore"):
        assert np.array_equal(h2 - want["image"]["hist"], want["image2"]["hist"])
    g.close()


def test_deposits_impulses_and_decode_on_one_stream_without_leaving_the_device():
    """hare_direct_device, hare_image_device and hare_image2_device into one per-sample third-order histogram, hare_hist_impulses_device on
    it with n0 = D, the band filters' delay, hare_decode_device on the rows: only the two decoded rows per receiver come down"""
    import torch
    case = oblique_case(3).without(n_bins=1500)
    want = pc.reference(case)
    wh, _ = summed(want, pc.ORDERS)
    g, _ = library_partition(case)
    K, nb, B, C = case.shape
    T, O, Td = 65, 2, 16
    taps = H.unit_energy_taps(H.band_taps(FS, [500.0, 2000.0], T))
    D = (T - 1) // 2
    n_out = nb
    h = np.random.default_rng(3).standard_normal((O, C, Td))
    P = case.P
    pairs, cands, paths = 1 << 12, 1 << 12, 1 << 15          # K x P = 336 pairs, P x P = 3 136 candidates, K x P x P = 18 816 paths at the most
    byt = lambda n: torch.zeros((int(n) + 7) // 8, dtype=torch.int64, device="cuda")
    w0, w1, w2 = byt(H.Voxel_Grid.direct_work_bytes(K)), byt(H.Voxel_Grid.image_work_bytes(K, P, pairs)), byt(H.Voxel_Grid.image2_work_bytes(P, cands, paths))
    d_hist = torch.zeros(K * nb * B * C, dtype=torch.int64, device="cuda")
    d_det = torch.zeros(2 * K, dtype=torch.int64, device="cuda")
    d_taps, d_h = torch.from_numpy(taps).to("cuda"), torch.from_numpy(h).to("cuda")
    d_rows = torch.full((K * C * n_out,), SENTINEL, dtype=torch.int64, device="cuda")
    Nd = n_out + Td - 1
    d_y = torch.full((K * O * Nd,), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    tail = (case.n_weight, nb, case.bin_len, case.frac_bits)
    kw = dict(directional=True, order=3, stream=stream)
    g.hist_impulses_device(1, 1, 1, 1, d_hist.data_ptr(), 0, 1, d_taps.data_ptr(), 0, 1, 1, 0, d_rows.data_ptr(), stream=stream)      # loads the module
    torch.cuda.synchronize()
    before = [g.get_option(o) for o in CALL_COUNTERS]
    g.direct_device(*tail, w0.data_ptr(), d_hist.data_ptr(), d_det.data_ptr(), **kw)
    g.Image_device(*tail, pairs, w1.data_ptr(), d_hist.data_ptr(), d_det.data_ptr(), **kw)
    g.Image2_device(*tail, cands, paths, w2.data_ptr(), d_hist.data_ptr(), d_det.data_ptr(), **kw)
    g.hist_impulses_device(K, nb, B, C, d_hist.data_ptr(), case.frac_bits, T, d_taps.data_ptr(), D, n_out, n_out, 0, d_rows.data_ptr(), stream=stream)
    g.decode_device(K, C, n_out, d_rows.data_ptr(), O, Td, d_h.data_ptr(), 0, Nd, d_y.data_ptr(), stream=stream)
    after = [g.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    assert after == before
    assert np.array_equal(d_hist.cpu().numpy().view(np.uint64).reshape(case.shape), wh)
    rows = impulse_ref(wh, taps, case.frac_bits, D, n_out)
    ref = decode_ref(rows, h)
    assert np.isfinite(ref).all() and ref.any()
    y = d_y.cpu().numpy().view(np.float64).reshape(K, O, Nd)
    assert same_bits(y, ref) is None, same_bits(y, ref)
    g.close()
