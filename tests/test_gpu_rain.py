"""Diffuse rain in the receive loop on the MI355X (include/hare_hip.h, "receivers", "Diffuse rain"): with HARE_RECEIVE_DIFFUSE_RAIN the
histogram, detections and final state equal, byte for byte, the numpy restatement (tests/receive_ref.py) whose shadow queries run through
the oracle's partition -- the shoebox, the hall and a room with an interior wall that occludes some of them; the three partitions; one band
and eight; one receiver, three and seventeen; the live-block list on and off.  Rain changes deposits only (rays and state are the call's
without it); without a scattering table, or with an all-zero one, it changes nothing; the sharded call is the one-device call; in a convex
room the expected totals are those without rain and the spread is smaller; the device call takes the enlarged work array and allocates
nothing."""
import numpy as np
import pytest

import hare_amd as H
from oracle import pyoracle as po
from tests.receive_ref import receive_loop
from tests.test_gpu_receivers import alpha_table, receivers
from tests.test_gpu_scattering import sigma_table

pytestmark = pytest.mark.gpu

BOUNCES = 5
N_BINS, BIN_LEN, FRAC = 600, 0.05, 40


def partition_room():
    """The shoebox (10 x 7 x 4) with an interior wall at x = 5 from y = 0 to 4.2, floor to ceiling: the burst source (x = 3.1) is on one
    side, a gap above y = 4.2 joins the two halves."""
    m = H.scenes.shoebox()
    wall = H.scenes._patch([5.0, 0.0, 0.0], [0.0, 4.2, 0.0], [0.0, 0.0, 4.0], 3, 3)
    v = np.zeros((wall.shape[0], 4, 3))
    v[:, :3] = wall
    return np.concatenate([m.verts, v]), np.concatenate([m.nverts, np.full(wall.shape[0], 3, np.int32)]), m.size


def partitions(verts, nverts, which=("voxel", "octree", "kdtree")):
    T, To = H.Topology(verts, nverts), po.Topology(verts, nverts)
    made = {"voxel": lambda: (H.Voxel_Grid([T], 8), po.VoxelGrid([To], domain=8)),
            "octree": lambda: (H.Octree([T], 4, 8), po.Octree([To], 4, 8)),
            "kdtree": lambda: (H.KDTree([T], 8, 6), po.KDTree([To], 8, 6))}
    return T, To, [made[w]() for w in which]


def check_rain(part, To, o, rays, centers, radii, B, seed, what, packs=(1, 0)):
    alpha = None if B == 1 else alpha_table(To.P, B)
    sigma = sigma_table(To.P, B)
    part.set_receivers(centers, radii)
    if alpha is not None:
        part.set_absorption(alpha)
    part.set_scattering(sigma)
    part.set_option("scatter_seed", seed)
    stats = {}
    want_h, want_d, want_s, _ = receive_loop(po, To, o, rays, BOUNCES, centers, radii, N_BINS, BIN_LEN, FRAC, alpha=alpha, sigma=sigma, seed=seed,
                                            rain=True, stats=stats)
    assert stats["eligible"] > 0 and want_d[:, 0].sum() > 0, what
    for pack in packs:
        part.set_option("bounce_pack", pack)
        hist, _, det, state, _ = part.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC, rain=True)
        tag = f"{what} B={B} K={len(centers)} pack={pack} n={len(rays)}"
        assert np.array_equal(det, want_d), (tag, det, want_d)
        assert np.array_equal(hist, want_h), (tag, np.argwhere(hist != want_h)[:5])
        assert state.tobytes() == want_s.tobytes(), tag
    part.set_option("bounce_pack", 1)
    return stats


def test_shoebox_three_partitions_bit_exact():
    m = H.scenes.shoebox()
    for n, B, K, packs in ((4097, 1, 1, (1, 0)), (65537, 8, 3, (1,))):
        T, To, parts = partitions(m.verts, m.nverts)       # fresh scenes per case: B changes
        c, r = receivers(m.size, K)
        rays = H.scenes.burst_rays(n, m.size)
        for part, o in parts:
            check_rain(part, To, o, rays, c, r, B, 11, f"shoebox {type(part).__name__}", packs)


def test_hall_bit_exact():
    m = H.scenes.hall()
    T, To = H.Topology(m.verts, m.nverts), po.Topology(m.verts, m.nverts)
    g, o = H.Voxel_Grid([T], 64), po.VoxelGrid([To], domain=64)
    c, r = receivers(m.size, K=3)
    check_rain(g, To, o, H.scenes.burst_rays(65537, m.size), c, r, 8, -4, "hall")
    c, r = receivers(m.size, K=17)
    g2 = H.Voxel_Grid([T], 64)
    check_rain(g2, To, o, H.scenes.burst_rays(4097, m.size), c, r, 1, 77, "hall", packs=(1,))


def test_interior_wall_occludes_some_queries_under_the_three_partitions():
    verts, nverts, size = partition_room()
    c = np.array([[7.5, 1.5, 2.0], [2.0, 5.0, 2.0], [7.0, 6.0, 1.5]])       # behind the wall, beside the source, past the gap
    r = np.array([0.5, 0.4, 0.6])
    rays = H.scenes.burst_rays(4097, size)
    T, To, parts = partitions(verts, nverts)
    for part, o in parts:
        stats = check_rain(part, To, o, rays, c, r, 8, 5, f"partition room {type(part).__name__}")
        assert 0 < stats["occluded"] < stats["eligible"], stats


def hall_grid(B=8):
    m = H.scenes.hall()
    T = H.Topology(m.verts, m.nverts)
    g = H.Voxel_Grid([T], 64)
    c, r = receivers(m.size, K=8)
    g.set_receivers(c, r).set_absorption(alpha_table(T.Polygon_Count, B))
    return m, T, g


def device_buffers(torch, n, K, B, rain):
    return dict(d_rays=torch.empty((n, 6), dtype=torch.float64, device="cuda"),
                d_state=torch.empty((1 + B, n), dtype=torch.float64, device="cuda"),
                d_work=torch.zeros(H.Voxel_Grid.receive_work_bytes(n, rain), dtype=torch.uint8, device="cuda"),
                d_last=torch.zeros(n * 56, dtype=torch.uint8, device="cuda"),
                d_hist=torch.zeros(K * N_BINS * B, dtype=torch.int64, device="cuda"),
                d_det=torch.zeros(2 * K, dtype=torch.int64, device="cuda"))


def run_device(torch, g, rays, B, rain, stream=None):
    n, K = len(rays), g.get_option("receivers")
    b = device_buffers(torch, n, K, B, rain)
    b["d_rays"].copy_(torch.from_numpy(rays))
    b["d_state"].copy_(torch.from_numpy(np.concatenate([np.zeros((1, n)), np.ones((B, n))])))
    torch.cuda.synchronize()
    before = [g.get_option(k) for k in ("hip_malloc_calls", "hip_free_calls", "hip_sync_calls")]
    g.receive_device(n, b["d_rays"].data_ptr(), BOUNCES, N_BINS, BIN_LEN, FRAC, b["d_state"].data_ptr(), b["d_work"].data_ptr(),
                     b["d_last"].data_ptr(), b["d_hist"].data_ptr(), b["d_det"].data_ptr(), stream=stream or 0, rain=rain)
    after = [g.get_option(k) for k in ("hip_malloc_calls", "hip_free_calls", "hip_sync_calls")]
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in b.items() if k != "d_work"}, before, after


def test_rain_changes_deposits_only():
    import torch
    m, T, g = hall_grid()
    g.set_scattering(sigma_table(T.Polygon_Count, 8)).set_option("scatter_seed", 12)
    rays = H.scenes.burst_rays(65537, m.size)
    plain = g.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC)
    rain = g.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC, rain=True)
    assert rain[3].tobytes() == plain[3].tobytes() and rain[4] == plain[4]          # state and counters
    assert not np.array_equal(rain[0], plain[0])
    # the final rays (every choice and direction) through the device call
    a, _, _ = run_device(torch, g, rays, 8, False)
    b, _, _ = run_device(torch, g, rays, 8, True)
    assert a["d_rays"].tobytes() == b["d_rays"].tobytes() and a["d_state"].tobytes() == b["d_state"].tobytes()
    assert a["d_last"].tobytes() == b["d_last"].tobytes()
    assert b["d_hist"].view(np.uint64).reshape(rain[0].shape).tobytes() == rain[0].tobytes()


def test_no_table_or_an_all_zero_one_changes_nothing():
    m, T, g = hall_grid()
    rays = H.scenes.burst_rays(65537, m.size)
    for table in (None, np.zeros((T.Polygon_Count, 8))):
        g.set_scattering(table)
        plain = g.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC)
        rain = g.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC, rain=True)
        for x, y in zip(plain[:4], rain[:4]):
            assert x.tobytes() == y.tobytes()
        assert plain[4] == rain[4]


def test_sharded_call_is_byte_identical():
    verts, nverts, size = partition_room()
    T = H.Topology(verts, nverts)
    parts = [H.Voxel_Grid([T], 8) for _ in range(2)]
    c, r = np.array([[7.5, 1.5, 2.0], [2.0, 5.0, 2.0]]), np.array([0.5, 0.4])
    a, s = alpha_table(T.Polygon_Count, 3), sigma_table(T.Polygon_Count, 3)
    for p in parts:
        p.set_receivers(c, r).set_absorption(a).set_scattering(s).set_option("scatter_seed", 8)
    rays = H.scenes.burst_rays(65537, size)
    one = parts[0].Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC, rain=True)
    two = H.Voxel_Grid.Receive_batch_sharded(parts, rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC, rain=True)
    for x, y in zip(one[:4], two[:4]):
        assert x.tobytes() == y.tobytes()
    assert one[4] == two[4]
    plain = parts[0].Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC)
    assert not np.array_equal(plain[0], one[0])


def test_convex_room_same_expected_totals_less_spread():
    m = H.scenes.shoebox()                                           # 10 x 7 x 4, convex
    T = H.Topology(m.verts, m.nverts)
    P, B, casts, seeds, n = T.Polygon_Count, 4, 4, 16, 1 << 17
    c = np.array([[3.0, 2.0, 2.0], [7.0, 5.0, 1.6]])                 # clear of every wall plane by 1.3 m or more
    r = np.array([0.3, 0.3])
    alpha = np.broadcast_to(np.array([0.05, 0.1, 0.2, 0.3]), (P, B)).copy()
    n_bins, bin_len = 1400, 0.05                                     # 70 m: every path of 4 casts lands in a bin
    late = int(12.0 / bin_len)                                       # after 12 m: reflections only
    rays = H.scenes.burst_rays(n, m.size)
    mixed = np.array([0.1, 0.4, 0.7, 0.95])
    for sigma in (np.ones((P, B)), np.broadcast_to(mixed, (P, B)).copy()):
        g = H.Voxel_Grid([T], 8)
        g.set_receivers(c, r).set_absorption(alpha).set_scattering(sigma)
        tot, spread = {}, {}
        for rain in (False, True):
            t, lt = [], []
            for seed in range(seeds):
                g.set_option("scatter_seed", 1000 + seed)
                _, hf, det, _, _ = g.Receive_batch(rays, casts, n_bins, bin_len, frac_bits=FRAC, rain=rain)
                assert det[:, 1].sum() == 0
                t.append(hf.sum(axis=(0, 1)))                        # per band, both receivers
                lt.append(hf[:, late:, :].sum(axis=(0, 1)))
            t, lt = np.array(t), np.array(lt)
            tot[rain] = (t.mean(0), t.std(0, ddof=1) / np.sqrt(seeds))
            spread[rain] = lt.std(0, ddof=1) / lt.mean(0)
        (m0, se0), (m1, se1) = tot[False], tot[True]
        assert np.all(np.abs(m1 - m0) < 5 * np.sqrt(se0 ** 2 + se1 ** 2)), (m0, m1, se0, se1)
        # rain removes the noise of the diffuse share; a band that reflects mostly specularly (sigma 0.1, 0.4) keeps the choice's noise
        diffuse = sigma[0] >= 0.5
        assert np.all(spread[True][diffuse] < spread[False][diffuse]), spread


def test_device_call_takes_the_enlarged_work_array_and_allocates_nothing():
    import torch
    m, T, g = hall_grid()
    g.set_scattering(sigma_table(T.Polygon_Count, 8)).set_option("scatter_seed", 31)
    rays = H.scenes.burst_rays(4159, m.size)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got, before, after = run_device(torch, g, rays, 8, True, stream=s.cuda_stream)
    assert after == before
    one = g.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC, rain=True)
    assert np.array_equal(got["d_hist"].view(np.uint64).reshape(one[0].shape), one[0])
    assert np.array_equal(got["d_det"].view(np.uint64).reshape(-1, 2), one[2])
    assert got["d_state"].tobytes() == one[3].tobytes()
