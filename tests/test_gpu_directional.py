"""Directional receivers on the MI355X (include/hare_hip.h, "receivers", "Directional"): with HARE_RECEIVE_DIRECTIONAL the four channels
of the histogram, the detections, the final state and the rays equal, byte for byte, the numpy restatement (tests/receive_ref.py)
-- the shoebox under the three partitions, the hall, the room whose interior wall occludes some of the rain's queries; one band and
eight; the live-block list on and off; the aggregated and the naive add; with no table, with a scattering table, with table and rain.
Channel 0, detections, state and rays are those of the call without the flag; the sharded call is the one-device call; the device call
accumulates into a four-fold histogram and allocates nothing; and the direct sound of a burst arrives from where the source is."""
import numpy as np
import pytest

import hare_amd as H
from oracle import pyoracle as po
from tests.receive_ref import receive_loop
from tests.test_gpu_rain import partition_room, partitions
from tests.test_gpu_receivers import alpha_table, receivers, source
from tests.test_gpu_scattering import sigma_table

pytestmark = pytest.mark.gpu

BOUNCES = 5
N_BINS, BIN_LEN, FRAC = 600, 0.05, 40
MODES = ("specular", "scatter", "rain")


def device_run(torch, g, rays, bounces, B, rain, directional, stream=None):
    """hare_receive_device from L = 0, E = 1 into zeroed accumulators: the buffers as numpy arrays and the allocation / wait counters
    before and after the call."""
    n, K = len(rays), g.get_option("receivers")
    b = dict(d_rays=torch.from_numpy(rays).to("cuda"),
             d_state=torch.from_numpy(np.concatenate([np.zeros((1, n)), np.ones((B, n))])).to("cuda"),
             d_work=torch.zeros(H.Voxel_Grid.receive_work_bytes(n, rain), dtype=torch.uint8, device="cuda"),
             d_last=torch.zeros(n * 56, dtype=torch.uint8, device="cuda"),
             d_hist=torch.zeros(K * N_BINS * B * (4 if directional else 1), dtype=torch.int64, device="cuda"),
             d_det=torch.zeros(2 * K, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    names = ("hip_malloc_calls", "hip_free_calls", "hip_sync_calls")
    before = [g.get_option(k) for k in names]
    g.receive_device(n, b["d_rays"].data_ptr(), bounces, N_BINS, BIN_LEN, FRAC, b["d_state"].data_ptr(), b["d_work"].data_ptr(),
                     b["d_last"].data_ptr(), b["d_hist"].data_ptr(), b["d_det"].data_ptr(), stream=stream or 0, rain=rain,
                     directional=directional)
    after = [g.get_option(k) for k in names]
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in b.items() if k != "d_work"}, before, after


def setup(part, P, centers, radii, B, seed, mode):
    alpha = None if B == 1 else alpha_table(P, B)
    sigma = None if mode == "specular" else sigma_table(P, B)
    part.set_receivers(centers, radii)
    if alpha is not None:
        part.set_absorption(alpha)
    part.set_scattering(sigma)
    part.set_option("scatter_seed", seed)
    return alpha, sigma


def check_directional(part, To, o, rays, centers, radii, B, seed, mode, what, packs=(1, 0), aggregates=(1, 0), device=True):
    import torch
    alpha, sigma = setup(part, To.P, centers, radii, B, seed, mode)
    rain = mode == "rain"
    stats = {}
    want_h, want_d, want_s, _ = receive_loop(po, To, o, rays, BOUNCES, centers, radii, N_BINS, BIN_LEN, FRAC, alpha=alpha, sigma=sigma, seed=seed,
                                            rain=rain, directional=True, stats=stats)
    assert want_d[:, 0].sum() > 0 and np.any(want_h[..., 1:] != 0), what
    if rain:
        assert stats["eligible"] > 0, what
    for pack in packs:
        for agg in aggregates:
            part.set_option("bounce_pack", pack).set_option("receive_aggregate", agg)
            hist, _, det, state, ctr = part.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC, rain=rain, directional=True)
            tag = f"{what} {mode} B={B} K={len(centers)} pack={pack} aggregate={agg} n={len(rays)}"
            assert hist.shape == want_h.shape and hist.dtype == np.uint64, tag
            assert np.array_equal(det, want_d), (tag, det, want_d)
            assert np.array_equal(hist, want_h), (tag, np.argwhere(hist != want_h)[:5])
            assert state.tobytes() == want_s.tobytes(), tag
            # the same call without the flag: channel 0, detections, state and counters are its own
            h0, _, d0, s0, c0 = part.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC, rain=rain)
            assert hist[..., 0].tobytes() == h0.tobytes() and det.tobytes() == d0.tobytes() and state.tobytes() == s0.tobytes(), tag
            assert ctr == c0, tag
    part.set_option("bounce_pack", 1).set_option("receive_aggregate", 1)
    if device:
        # the rays: two casts (every ray of the burst is reflected once), through the device call, with and without the flag
        *_, want_rays = receive_loop(po, To, o, rays, 2, centers, radii, N_BINS, BIN_LEN, FRAC, alpha=alpha, sigma=sigma, seed=seed, rain=rain,
                                     directional=True)
        a, _, _ = device_run(torch, part, rays, 2, B, rain, True)
        b, _, _ = device_run(torch, part, rays, 2, B, rain, False)
        assert a["d_rays"].tobytes() == want_rays.tobytes(), (what, mode, np.argwhere(a["d_rays"] != want_rays)[:5])
        for k in ("d_rays", "d_state", "d_last", "d_det"):
            assert a[k].tobytes() == b[k].tobytes(), (what, mode, k)
        assert a["d_hist"].reshape(-1, 4)[:, 0].tobytes() == b["d_hist"].tobytes(), (what, mode)
    return stats


def test_shoebox_three_partitions_bit_exact():
    m = H.scenes.shoebox()
    for n, B, K, packs, aggs in ((4097, 1, 1, (1, 0), (1, 0)), (4159, 8, 3, (1, 0), (1, 0)), (65537, 8, 3, (1,), (1, 0))):
        c, r = receivers(m.size, K)
        rays = H.scenes.burst_rays(n, m.size)
        for mode in MODES:
            T, To, parts = partitions(m.verts, m.nverts)       # fresh scenes per case: B and the tables change
            for part, o in parts:
                check_directional(part, To, o, rays, c, r, B, 11, mode, f"shoebox {type(part).__name__}", packs, aggs,
                                  device=type(part).__name__ == "Voxel_Grid")


def test_hall_bit_exact():
    m = H.scenes.hall()
    T, To = H.Topology(m.verts, m.nverts), po.Topology(m.verts, m.nverts)
    o = po.VoxelGrid([To], domain=64)
    for n, B, K, seed, packs in ((65537, 8, 3, -4, (1, 0)), (4097, 1, 17, 77, (1,))):
        c, r = receivers(m.size, K)
        rays = H.scenes.burst_rays(n, m.size)
        for mode in MODES:
            check_directional(H.Voxel_Grid([T], 64), To, o, rays, c, r, B, seed, mode, "hall", packs)


def test_interior_wall_with_rain_under_the_three_partitions():
    verts, nverts, size = partition_room()
    c = np.array([[7.5, 1.5, 2.0], [2.0, 5.0, 2.0], [7.0, 6.0, 1.5]])       # behind the wall, beside the source, past the gap
    r = np.array([0.5, 0.4, 0.6])
    for n, B in ((4097, 8), (4159, 1)):
        rays = H.scenes.burst_rays(n, size)
        T, To, parts = partitions(verts, nverts)
        for part, o in parts:
            stats = check_directional(part, To, o, rays, c, r, B, 5, "rain", f"partition room {type(part).__name__}", device=False)
            assert 0 < stats["occluded"] < stats["eligible"], stats


def test_sharded_call_is_byte_identical():
    verts, nverts, size = partition_room()
    T = H.Topology(verts, nverts)
    parts = [H.Voxel_Grid([T], 8) for _ in range(2)]
    c, r = np.array([[7.5, 1.5, 2.0], [2.0, 5.0, 2.0]]), np.array([0.5, 0.4])
    a, s = alpha_table(T.Polygon_Count, 3), sigma_table(T.Polygon_Count, 3)
    for p in parts:
        p.set_receivers(c, r).set_absorption(a).set_option("scatter_seed", 8)
    rays = H.scenes.burst_rays(65537, size)
    for mode in MODES:
        for p in parts:
            p.set_scattering(None if mode == "specular" else s)
        rain = mode == "rain"
        one = parts[0].Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC, rain=rain, directional=True)
        two = H.Voxel_Grid.Receive_batch_sharded(parts, rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC, rain=rain, directional=True)
        assert one[0].shape == (2, N_BINS, 3, 4) and np.any(H.Voxel_Grid.directional_signed(one[0]) < 0), mode
        for x, y in zip(one[:4], two[:4]):
            assert x.tobytes() == y.tobytes(), mode
        assert one[4] == two[4], mode
        out = np.full((2, N_BINS, 3, 4), 99, np.uint64)               # the caller's array is written, not accumulated into
        again = H.Voxel_Grid.Receive_batch_sharded(parts, rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC, rain=rain, directional=True, out=out)
        assert again[0] is out and out.tobytes() == one[0].tobytes(), mode


def test_device_call_accumulates_into_the_four_fold_histogram_and_allocates_nothing():
    import torch
    m = H.scenes.hall()
    T = H.Topology(m.verts, m.nverts)
    g = H.Voxel_Grid([T], 64)
    c, r = receivers(m.size, K=8)
    g.set_receivers(c, r).set_absorption(alpha_table(T.Polygon_Count, 8))
    g.set_scattering(sigma_table(T.Polygon_Count, 8)).set_option("scatter_seed", 31)
    rays = H.scenes.burst_rays(4159, m.size)
    for rain in (False, True):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            got, before, after = device_run(torch, g, rays, BOUNCES, 8, rain, True, stream=s.cuda_stream)
        assert after == before, rain
        one = g.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC, rain=rain, directional=True)
        assert np.array_equal(got["d_hist"].view(np.uint64).reshape(one[0].shape), one[0]), rain
        assert np.array_equal(got["d_det"].view(np.uint64).reshape(-1, 2), one[2]), rain
        assert got["d_state"].tobytes() == one[3].tobytes(), rain
    # accumulated: a second call into the same buffers doubles every word (wrapping adds of two's-complement words)
    n, K, B = len(rays), 8, 8
    d_hist = torch.zeros(K * N_BINS * B * 4, dtype=torch.int64, device="cuda")
    d_det = torch.zeros(2 * K, dtype=torch.int64, device="cuda")
    d_work = torch.zeros(H.Voxel_Grid.receive_work_bytes(n, True), dtype=torch.uint8, device="cuda")
    d_last = torch.zeros(n * 56, dtype=torch.uint8, device="cuda")
    for _ in range(2):
        d_rays = torch.from_numpy(rays).to("cuda")
        d_state = torch.from_numpy(np.concatenate([np.zeros((1, n)), np.ones((B, n))])).to("cuda")
        g.receive_device(n, d_rays.data_ptr(), BOUNCES, N_BINS, BIN_LEN, FRAC, d_state.data_ptr(), d_work.data_ptr(), d_last.data_ptr(),
                         d_hist.data_ptr(), d_det.data_ptr(), rain=True, directional=True)
        torch.cuda.synchronize()
    assert np.array_equal(d_hist.cpu().numpy().reshape(one[0].shape), 2 * one[0].view(np.int64))
    assert np.array_equal(d_det.cpu().numpy().view(np.uint64).reshape(-1, 2), 2 * one[2])


def test_direct_sound_arrives_from_the_source():
    """bounces = 1, a burst from S, one receiver of radius 1 m centred at S + (2, 0, 0), one bin of 4 m.  A detected ray passes within
    1 m of a point 2 m away, so it travels within 30 degrees of +x (sin < 1/2): its a_x lies in [-1, -cos 30], and cos 30 > 0.866.
    Summed over the bin: X < 0 and 0.866 W - detections <= -X <= W + detections (every rint moves a word by at most 1/2)."""
    m = H.scenes.shoebox()                                           # 10 x 7 x 4; S = (3.1, 2.94, 1.48): the sphere is clear of every wall
    S = source(m.size)
    assert np.all(S + [2.0, 0.0, 0.0] - 1.0 > 0.4) and np.all(S + [2.0, 0.0, 0.0] + 1.0 < np.asarray(m.size) - 0.4)
    rays = H.scenes.burst_rays(65537, m.size)
    for part in (H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8), H.Octree([H.Topology(m.verts, m.nverts)], 4, 8)):
        part.set_receivers([S + [2.0, 0.0, 0.0]], [1.0])
        for agg in (1, 0):
            part.set_option("receive_aggregate", agg)
            hist, _, det, _, _ = part.Receive_batch(rays, 1, 1, 4.0, frac_bits=FRAC, directional=True)
            W = int(hist[0, 0, 0, 0])
            X, Y, Z = (int(v) for v in H.Voxel_Grid.directional_signed(hist)[0, 0, 0])
            D = int(det[0, 0])
            print(f"directional direct sound: W {W} X {X} Y {Y} Z {Z} detections {D} (-X / W = {-X / W:.6f})")
            # the cap of half-angle 30 degrees holds (1 - cos 30) / 2 = 6.7 % of the sphere: about 4 390 of 65 537 rays
            assert det[0, 1] == 0 and 4000 < D < 4800 and W == D << FRAC
            assert X < 0
            assert 1000 * -X >= 866 * W - 1000 * D
            assert -X <= W + D
            # the cap is symmetric about the x axis: the transverse sums nearly cancel (each ray's |a_y|, |a_z| < 1/2)
            assert 2 * abs(Y) <= W + 2 * D and 2 * abs(Z) <= W + 2 * D
