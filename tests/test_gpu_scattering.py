"""Diffuse scattering in the receive loop on the MI355X (include/hare_hip.h, "receivers", "Scattering"): hare_receive_scatter's histogram,
detections and final ray state must equal, byte for byte, the numpy restatement (tests/receive_ref.py) run cast by cast on the oracle's
partition -- closed rooms and an open soup, the three partitions, one band and eight with rows of 0 and 1, the live-block list on and off,
batch sizes that are not a multiple of 4.  An all-zero table is no table; the scattered rays themselves match and obey the cosine law;
the same seed gives the same bytes and another seed another histogram; the sharded call is the one-device call; the device call allocates,
frees and waits for nothing."""
import numpy as np
import pytest

import hare_amd as H
from oracle import pyoracle as po
from tests.helpers import soup, soup_rays
from tests.receive_ref import receive_loop
from tests.scatter_ref import normals_of
from tests.test_gpu_receivers import alpha_table, receivers

pytestmark = pytest.mark.gpu

BOUNCES = 6
N_BINS, BIN_LEN, FRAC = 400, 0.05, 40


def sigma_table(P, B, seed=3):
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.0, 1.0, (P, B))
    s[::13] = 0.0                                                    # specular polygons
    s[4::19] = 1.0                                                   # fully diffuse ones
    if B > 1:
        s[7::11, 0] = 0.0                                            # uneven rows: a band that never scatters beside one that always does
        s[7::11, B - 1] = 1.0
    return s


def check_scatter(part, To, o, rays, centers, radii, B, seed, what, packs=(1, 0)):
    alpha = None if B == 1 else alpha_table(To.P, B)
    sigma = sigma_table(To.P, B)
    part.set_receivers(centers, radii)
    if alpha is not None:
        part.set_absorption(alpha)
    part.set_scattering(sigma)
    part.set_option("scatter_seed", seed)
    want_h, want_d, want_s, _ = receive_loop(po, To, o, rays, BOUNCES, centers, radii, N_BINS, BIN_LEN, FRAC, alpha=alpha, sigma=sigma, seed=seed)
    assert want_d[:, 0].sum() > 0, what
    for pack in packs:
        part.set_option("bounce_pack", pack)
        hist, _, det, state, _ = part.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC)
        tag = f"{what} B={B} pack={pack} n={len(rays)}"
        assert np.array_equal(det, want_d), (tag, det, want_d)
        assert np.array_equal(hist, want_h), (tag, np.argwhere(hist != want_h)[:5])
        assert state.tobytes() == want_s.tobytes(), (tag, np.argwhere(state != want_s)[:5])
    part.set_option("bounce_pack", 1)
    return want_h, want_d, want_s


def room(name, domain):
    m = getattr(H.scenes, name)()
    T, To = H.Topology(m.verts, m.nverts), po.Topology(m.verts, m.nverts)
    return m, T, To, H.Voxel_Grid([T], domain), po.VoxelGrid([To], domain=domain)


def test_shoebox_one_and_eight_bands_bit_exact():
    for n, B, seed in ((4097, 1, 0), (4159, 8, -5), (65537, 8, 1 << 40), (65537, 1, 17)):
        m, T, To, g, o = room("shoebox", 8)                          # a fresh scene per case: B changes from case to case
        c, r = receivers(m.size)
        check_scatter(g, To, o, H.scenes.burst_rays(n, m.size), c, r, B, seed, "shoebox")


def test_hall_eight_bands_bit_exact():
    m, T, To, g, o = room("hall", 64)
    c, r = receivers(m.size, K=8)
    check_scatter(g, To, o, H.scenes.burst_rays(65537, m.size), c, r, 8, 123456789, "hall")


def test_hall_one_band_bit_exact():
    m, T, To, g, o = room("hall", 64)
    c, r = receivers(m.size, K=8)
    check_scatter(g, To, o, H.scenes.burst_rays(4159, m.size), c, r, 1, -1, "hall", packs=(1,))


def test_open_soup_under_the_three_partitions():
    verts, nverts, size = soup()
    T, To = H.Topology(verts, nverts), po.Topology(verts, nverts)
    c, r = receivers(size, K=6)
    c[5] = (-3.0, 2.5, 2.0)                                          # outside the model: only escaped rays reach it
    r[5] = 1.5
    for n in (4097, 4159):
        rays = soup_rays(n, size)
        for part, orc in ((H.Voxel_Grid([T], 12), po.VoxelGrid([To], domain=12)), (H.Octree([T], 4, 8), po.Octree([To], 4, 8)),
                          (H.KDTree([T], 8, 6), po.KDTree([To], 8, 6))):
            check_scatter(part, To, orc, rays, c, r, 8 if n == 4159 else 1, 99, type(part).__name__)


def test_all_zero_table_is_no_table():
    m, T, To, g, o = room("hall", 64)
    c, r = receivers(m.size, K=8)
    rays = H.scenes.burst_rays(65537, m.size)
    a = alpha_table(T.Polygon_Count, 8)
    g.set_receivers(c, r).set_absorption(a)
    plain = g.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC)
    g.set_scattering(np.zeros((T.Polygon_Count, 8))).set_option("scatter_seed", 42)
    zero = g.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC)
    for x, y in zip(plain[:4], zero[:4]):
        assert x.tobytes() == y.tobytes()
    assert plain[4] == zero[4]


def device_buffers(torch, n, K, B):
    return dict(d_rays=torch.empty((n, 6), dtype=torch.float64, device="cuda"),
                d_state=torch.empty((1 + B, n), dtype=torch.float64, device="cuda"),
                d_work=torch.zeros(2 * n, dtype=torch.int32, device="cuda"),
                d_last=torch.zeros(n * 56, dtype=torch.uint8, device="cuda"),
                d_hist=torch.zeros(K * N_BINS * B, dtype=torch.int64, device="cuda"),
                d_det=torch.zeros(2 * K, dtype=torch.int64, device="cuda"))


def test_scattered_rays_match_and_follow_the_cosine_law():
    import torch
    m, T, To, g, o = room("hall", 64)
    c, r = receivers(m.size, K=8)
    n, B = 65537, 8
    rays = H.scenes.burst_rays(n, m.size)
    g.set_receivers(c, r)
    for sigma, seed in ((sigma_table(T.Polygon_Count, B), 5), (np.ones((T.Polygon_Count, B)), -77)):
        g.set_scattering(sigma).set_option("scatter_seed", seed)
        _, _, want_s, want_rays = receive_loop(po, To, o, rays, 2, c, r, N_BINS, BIN_LEN, FRAC, sigma=sigma, seed=seed, keep_rays_after=0)
        b = device_buffers(torch, n, len(c), B)
        b["d_rays"].copy_(torch.from_numpy(rays))
        b["d_state"].copy_(torch.from_numpy(np.concatenate([np.zeros((1, n)), np.ones((B, n))])))
        torch.cuda.synchronize()
        g.receive_device(n, b["d_rays"].data_ptr(), 2, N_BINS, BIN_LEN, FRAC, b["d_state"].data_ptr(), b["d_work"].data_ptr(),
                         b["d_last"].data_ptr(), b["d_hist"].data_ptr(), b["d_det"].data_ptr())
        torch.cuda.synchronize()
        got = b["d_rays"].cpu().numpy()
        assert got.tobytes() == want_rays.tobytes(), np.argwhere(got != want_rays)[:5]
        assert b["d_state"].cpu().numpy().tobytes() == want_s.tobytes()
    # sigma = 1 everywhere: every ray that hit in cast 0 left diffusely, cosine-distributed about the normal on its side
    ev0, _ = o.shoot(rays, nthreads=16)
    hit = ev0["hit"] == 1
    nrm = normals_of(To)[ev0["poly_id"][hit]]
    d_in = rays[hit, 3:]
    nprime = np.where(((d_in * nrm).sum(1) > 0)[:, None], -nrm, nrm)
    d_out = got[hit, 3:]
    cos = (d_out * nprime).sum(1) / np.linalg.norm(d_out, axis=1)
    assert hit.sum() > 0.9 * n and np.all(cos >= 0)
    assert abs(cos.mean() - 2.0 / 3.0) < 0.005
    assert np.array_equal(got[hit, :3], np.stack([ev0["x"], ev0["y"], ev0["z"]], 1)[hit])


def test_same_seed_same_bytes_other_seed_other_histogram():
    m, T, To, g, o = room("hall", 64)
    c, r = receivers(m.size, K=8)
    rays = H.scenes.burst_rays(65537, m.size)
    g.set_receivers(c, r).set_absorption(alpha_table(T.Polygon_Count, 8)).set_scattering(sigma_table(T.Polygon_Count, 8))
    g.set_option("scatter_seed", 2024)
    one = g.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC)
    two = g.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC)
    for x, y in zip(one[:4], two[:4]):
        assert x.tobytes() == y.tobytes()
    g.set_option("scatter_seed", 2025)
    other = g.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC)
    assert not np.array_equal(other[0], one[0])
    assert other[3].tobytes() != one[3].tobytes()


def test_sharded_call_is_byte_identical_and_refuses_differing_scenes():
    m = H.scenes.shoebox()
    T = H.Topology(m.verts, m.nverts)
    parts = [H.Voxel_Grid([T], 8) for _ in range(2)]
    c, r = receivers(m.size)
    a, s = alpha_table(T.Polygon_Count, 3), sigma_table(T.Polygon_Count, 3)
    for p in parts:
        p.set_receivers(c, r).set_absorption(a).set_scattering(s).set_option("scatter_seed", -9)
    n = 65537
    rays = H.scenes.burst_rays(n, m.size)
    one = parts[0].Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC)
    two = H.Voxel_Grid.Receive_batch_sharded(parts, rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC)
    for x, y in zip(one[:4], two[:4]):
        assert x.tobytes() == y.tobytes()
    To = po.Topology(m.verts, m.nverts)
    want_h, want_d, want_s, _ = receive_loop(po, To, po.VoxelGrid([To], domain=8), rays, BOUNCES, c, r, N_BINS, BIN_LEN, FRAC, alpha=a, sigma=s,
                                            seed=-9)
    assert np.array_equal(one[0], want_h) and np.array_equal(one[2], want_d) and one[3].tobytes() == want_s.tobytes()
    # the scenes must scatter alike: another seed, another table, no table
    for change, undo in ((lambda: parts[1].set_option("scatter_seed", 3), lambda: parts[1].set_option("scatter_seed", -9)),
                         (lambda: parts[1].set_scattering(s * 0.5), lambda: parts[1].set_scattering(s)),
                         (lambda: parts[1].set_scattering(None), lambda: parts[1].set_scattering(s))):
        change()
        with pytest.raises(H.HareError) as ei:
            H.Voxel_Grid.Receive_batch_sharded(parts, rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC)
        assert ei.value.code == H.capi.HARE_E_INVALID
        undo()
    again = H.Voxel_Grid.Receive_batch_sharded(parts, rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC)
    assert again[0].tobytes() == one[0].tobytes()


def test_device_call_allocates_nothing():
    import torch
    m, T, To, g, o = room("hall", 64)
    c, r = receivers(m.size, K=8)
    B, n = 8, 4159
    g.set_receivers(c, r).set_absorption(alpha_table(T.Polygon_Count, B)).set_scattering(sigma_table(T.Polygon_Count, B))
    g.set_option("scatter_seed", 31)
    rays = H.scenes.burst_rays(n, m.size)
    b = device_buffers(torch, n, len(c), B)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b["d_rays"].copy_(torch.from_numpy(rays))
        b["d_state"].copy_(torch.from_numpy(np.concatenate([np.zeros((1, n)), np.ones((B, n))])))
        torch.cuda.synchronize()
        before = [g.get_option(k) for k in ("hip_malloc_calls", "hip_free_calls", "hip_sync_calls")]
        g.receive_device(n, b["d_rays"].data_ptr(), BOUNCES, N_BINS, BIN_LEN, FRAC, b["d_state"].data_ptr(), b["d_work"].data_ptr(),
                         b["d_last"].data_ptr(), b["d_hist"].data_ptr(), b["d_det"].data_ptr(), stream=s.cuda_stream)
        assert [g.get_option(k) for k in ("hip_malloc_calls", "hip_free_calls", "hip_sync_calls")] == before
        s.synchronize()
    hist = b["d_hist"].cpu().numpy().view(np.uint64).reshape(len(c), N_BINS, B)
    one = g.Receive_batch(rays, BOUNCES, N_BINS, BIN_LEN, frac_bits=FRAC)
    assert np.array_equal(hist, one[0]) and b["d_state"].cpu().numpy().tobytes() == one[3].tobytes()
