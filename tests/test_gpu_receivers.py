"""Receivers on the MI355X (include/hare_hip.h, "receivers"): the energy-time histogram, the detections and the final ray state of the
receive loop must equal, bit for bit, the numpy restatement (tests/receive_ref.py) run on the oracle's bounce loop (every cast's events
from tests.helpers.oracle_bounce_loop, every cast's rays rebuilt with the oracle's reflection).  Closed rooms (the shoebox, the hall) with
receivers near and far from a burst source, an open soup where rays escape and half-lines count; the three partitions; one band and
eight; the live-block list on and off; the fused-loop option on and off (the receive loop never fuses); batch sizes that are not a
multiple of 4 (the live-block bytes' alignment).  The sharded call, the device call's accumulation and its promise to allocate nothing."""
import numpy as np
import pytest

import hare_amd as H
from oracle import pyoracle as po
from tests.helpers import oracle_bounce_loop, soup, soup_rays
from tests.receive_ref import replay_loop

pytestmark = pytest.mark.gpu

BOUNCES = 6
N_BINS, BIN_LEN, FRAC = 400, 0.05, 40


def source(size):
    return np.array([0.31, 0.42, 0.37]) * np.asarray(size)          # hare_amd.scenes.burst_rays


def receivers(size, K=5):
    """Receiver 0 a metre from the source (the direct sound piles onto one or two bins), the others spread over the room."""
    S, L = source(size), np.asarray(size, float)
    c = [S + np.array([1.0, 0.0, 0.0])]
    rng = np.random.default_rng(7)
    c += list(rng.uniform(0.15, 0.85, (K - 1, 3)) * L)
    r = np.concatenate([[0.5], rng.uniform(0.2, 0.9, K - 1)])
    return np.array(c), r


def alpha_table(P, B, seed=2):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 0.6, (P, B))
    a[::17] = 0.0
    a[5::23] = 1.0                                                   # full absorption: the ray carries nothing on, but lives on
    return a


def check_receive(part, To, o, rays, centers, radii, B, what, combos, state_in=None):
    ref_ev, _ = oracle_bounce_loop(po, To, o, rays, BOUNCES)
    alpha = None if B == 1 else alpha_table(To.P, B)
    part.set_receivers(centers, radii)
    if alpha is not None:
        part.set_absorption(alpha)
    want_h, want_d, want_s = replay_loop(po, To, rays, ref_ev, centers, radii, N_BINS, BIN_LEN, FRAC, alpha=alpha, state_in=state_in)
    assert want_d[:, 0].sum() > 0, what                              # the case detects something
    for pack, fused in combos:
        part.set_option("bounce_pack", pack)
        part.set_option("bounce_fused", fused)
        hist, histf, det, state, ctr = part.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, energy=state_in, frac_bits=FRAC)
        tag = f"{what} B={B} pack={pack} fused={fused} n={len(rays)}"
        assert hist.shape == (len(centers), N_BINS, B), tag
        assert np.array_equal(det, want_d), (tag, det, want_d)
        assert np.array_equal(hist, want_h), (tag, np.argwhere(hist != want_h)[:5])
        assert state.tobytes() == want_s.tobytes(), tag
        assert np.array_equal(histf, hist.astype(np.float64) * 2.0 ** -FRAC), tag
    part.set_option("bounce_pack", 1)
    part.set_option("bounce_fused", 0)
    return want_h, want_d, want_s


def test_shoebox_near_and_far_receivers_one_and_eight_bands():
    m = H.scenes.shoebox()
    T, To = H.Topology(m.verts, m.nverts), po.Topology(m.verts, m.nverts)
    g, o = H.Voxel_Grid([T], 8), po.VoxelGrid([To], domain=8)
    c, r = receivers(m.size)
    for n, B, combos in ((4097, 1, ((1, 0), (0, 1))), (4159, 8, ((1, 1), (0, 0))), (65537, 8, ((1, 0), (0, 1)))):
        check_receive(g, To, o, H.scenes.burst_rays(n, m.size), c, r, B, "shoebox", combos)


def test_hall_burst_with_direct_sound():
    m = H.scenes.hall()
    T, To = H.Topology(m.verts, m.nverts), po.Topology(m.verts, m.nverts)
    g, o = H.Voxel_Grid([T], 64), po.VoxelGrid([To], domain=64)
    c, r = receivers(m.size, K=8)
    rays = H.scenes.burst_rays(65537, m.size)
    check_receive(g, To, o, rays, c, r, 8, "hall", ((1, 0), (0, 1)))
    g.set_option("receive_aggregate", 0)                              # the naive atomics: the same sums
    check_receive(g, To, o, rays, c, r, 8, "hall naive", ((1, 0),))
    g.set_option("receive_aggregate", 1)


def test_open_soup_half_lines_and_the_three_partitions():
    verts, nverts, size = soup()
    T, To = H.Topology(verts, nverts), po.Topology(verts, nverts)
    c, r = receivers(size, K=6)
    c[5] = (-3.0, 2.5, 2.0)                                          # outside the model: only escaped rays (half-lines) reach it
    r[5] = 1.5
    for n in (4097, 4159):
        rays = soup_rays(n, size)
        for part, orc in ((H.Voxel_Grid([T], 12), po.VoxelGrid([To], domain=12)), (H.Octree([T], 4, 8), po.Octree([To], 4, 8)),
                          (H.KDTree([T], 8, 6), po.KDTree([To], 8, 6))):
            _, want_d, _ = check_receive(part, To, orc, rays, c, r, 8 if n == 4159 else 1, type(part).__name__, ((1, 0), (0, 1)))
            assert want_d[5].sum() > 0


def test_sharded_call_is_byte_identical_and_state_in_is_read():
    m = H.scenes.shoebox()
    T = H.Topology(m.verts, m.nverts)
    parts = [H.Voxel_Grid([T], 8) for _ in range(2)]
    c, r = receivers(m.size)
    a = alpha_table(T.Polygon_Count, 3)
    for p in parts:
        p.set_receivers(c, r).set_absorption(a)
    n = 65537
    rays = H.scenes.burst_rays(n, m.size)
    rng = np.random.default_rng(4)
    st = np.concatenate([rng.uniform(0, 3, (1, n)), rng.uniform(0, 2, (3, n))])
    one = parts[0].Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, energy=st, frac_bits=FRAC)
    two = H.Voxel_Grid.Receive_batch_sharded(parts, rays, BOUNCES, N_BINS, BIN_LEN, energy=st, frac_bits=FRAC)
    for x, y in zip(one[:4], two[:4]):
        assert x.tobytes() == y.tobytes()
    assert one[4]["hits"] == two[4]["hits"]
    To, o = po.Topology(m.verts, m.nverts), po.VoxelGrid([po.Topology(m.verts, m.nverts)], domain=8)
    ref_ev, _ = oracle_bounce_loop(po, To, o, rays, BOUNCES)
    want_h, want_d, want_s = replay_loop(po, To, rays, ref_ev, c, r, N_BINS, BIN_LEN, FRAC, alpha=a, state_in=st)
    assert np.array_equal(one[0], want_h) and np.array_equal(one[2], want_d) and one[3].tobytes() == want_s.tobytes()
    out = np.zeros_like(one[0])
    again = parts[1].Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, energy=st, frac_bits=FRAC, out=out)
    assert again[0] is out and out.tobytes() == one[0].tobytes()


def test_device_call_accumulates_on_a_torch_stream_and_allocates_nothing():
    import torch
    m = H.scenes.hall()
    T, To = H.Topology(m.verts, m.nverts), po.Topology(m.verts, m.nverts)
    g = H.Voxel_Grid([T], 64)
    c, r = receivers(m.size, K=8)
    B = 8
    a = alpha_table(T.Polygon_Count, B)
    g.set_receivers(c, r).set_absorption(a)
    n = 4159
    rays = H.scenes.burst_rays(n, m.size)
    K = len(c)
    d_rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    d_state = torch.empty((1 + B, n), dtype=torch.float64, device="cuda")
    d_work = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    d_last = torch.zeros(n * 56, dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros(K * N_BINS * B, dtype=torch.int64, device="cuda")
    d_det = torch.zeros(2 * K, dtype=torch.int64, device="cuda")
    d_ctr = torch.zeros(8, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    init = np.concatenate([np.zeros((1, n)), np.ones((B, n))])
    states = []
    with torch.cuda.stream(s):
        for _ in range(2):
            d_rays.copy_(torch.from_numpy(rays))
            d_state.copy_(torch.from_numpy(init))
            torch.cuda.synchronize()
            before = [g.get_option(k) for k in ("hip_malloc_calls", "hip_free_calls", "hip_sync_calls")]
            g.receive_device(n, d_rays.data_ptr(), BOUNCES, N_BINS, BIN_LEN, FRAC, d_state.data_ptr(), d_work.data_ptr(), d_last.data_ptr(),
                             d_hist.data_ptr(), d_det.data_ptr(), d_counters=d_ctr.data_ptr(), stream=s.cuda_stream)
            assert [g.get_option(k) for k in ("hip_malloc_calls", "hip_free_calls", "hip_sync_calls")] == before
            s.synchronize()
            states.append(d_state.cpu().numpy().copy())
    hist = d_hist.cpu().numpy().view(np.uint64).reshape(K, N_BINS, B)
    det = d_det.cpu().numpy().view(np.uint64).reshape(K, 2)
    one, one_f, one_d, one_s, ctr = g.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC)
    assert np.array_equal(hist, one * np.uint64(2)) and np.array_equal(det, one_d * np.uint64(2))
    assert states[0].tobytes() == one_s.tobytes() and states[1].tobytes() == one_s.tobytes()
    assert int(d_ctr.cpu().numpy()[1]) == 2 * ctr["hits"]
    ref_ev, _ = oracle_bounce_loop(po, To, po.VoxelGrid([To], domain=64), rays, BOUNCES)
    want_h, want_d, _ = replay_loop(po, To, rays, ref_ev, c, r, N_BINS, BIN_LEN, FRAC, alpha=a)
    assert np.array_equal(one, want_h) and np.array_equal(one_d, want_d)
    last = np.frombuffer(d_last.cpu().numpy().tobytes(), H.capi.XEVENT_DTYPE)
    assert last.tobytes() == ref_ev[BOUNCES - 1].tobytes()
