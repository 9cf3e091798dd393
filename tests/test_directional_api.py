"""Directional receivers (include/hare_hip.h, "receivers", "Directional") without a GPU: the flag is a bit of its own and every binding
repeats it; the numpy restatement the GPU tests compare against (tests/receive_ref.py) gives the hand-worked words for two rays and
one rain deposit, its channel 0 is the omni restatements' histogram word for word and its signed channels stay within channel 0 plus
the adds; the argument checks that need no device see the four-fold histogram; the C++ mirror passes the flag."""
import os
import re
import subprocess

import numpy as np

import hare_amd as H
from hare_amd import capi
from oracle import pyoracle as po
from tests.helpers import oracle_bounce_loop
from tests.receive_ref import receive_loop, receiver_step_dir, replay_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hare_hip.h")


def header_defines():
    return {k: int(v) for k, v in re.findall(r"#define\s+(HARE_[A-Z_]+)\s+(\d+)u", open(HEADER).read())}


def test_flag_is_a_bit_of_its_own_and_bound_everywhere():
    d = header_defines()
    flag = d["HARE_RECEIVE_DIRECTIONAL"]
    assert flag == 256 == capi.RECEIVE_DIRECTIONAL and flag & (flag - 1) == 0
    others = [v for k, v in d.items() if (k.startswith("HARE_SHOOT_") or k.startswith("HARE_RECEIVE_")) and k != "HARE_RECEIVE_DIRECTIONAL"]
    assert len(others) >= 8 and d["HARE_RECEIVE_DIFFUSE_RAIN"] in others and all(v & flag == 0 for v in others)
    assert flag & (0xF000 | 0x40000 | 0x80000) == 0                 # the developer bits and the internal ones (launch.cpp asserts it too)
    launch = open(os.path.join(ROOT, "hare_amd", "csrc", "launch.cpp")).read()
    assert "static_assert((HARE_RECEIVE_DIRECTIONAL &" in launch
    hpp = open(os.path.join(ROOT, "bindings", "cpp", "hare.hpp")).read()
    assert "bool rain = false, bool directional = false)" in hpp and "directional ? HARE_RECEIVE_DIRECTIONAL : 0u" in hpp
    cs = open(os.path.join(ROOT, "bindings", "csharp", "HareHip.cs")).read()
    assert re.search(r"HARE_RECEIVE_DIRECTIONAL\s*=\s*256\s*;", cs)
    part = open(os.path.join(ROOT, "bindings", "csharp", "Gpu_Spatial_Partition.cs")).read()
    assert re.search(r"public long Receive\([^)]*bool state_in, bool rain, bool directional\)", part)
    assert "directional ? HareHip.HARE_RECEIVE_DIRECTIONAL : 0u" in part
    for fn in (H.Voxel_Grid.Receive_batch, H.Voxel_Grid.Receive_batch_sharded, H.Voxel_Grid.receive_device):
        names = fn.__code__.co_varnames[:fn.__code__.co_argcount]
        assert "directional" in names and names.index("directional") == names.index("rain") + 1, fn
        assert fn.__defaults__[-1] is False                          # opt-in


def test_signed_view_and_shape():
    h = np.zeros((2, 3, 4, 4), np.uint64)
    h[1, 2, 3] = [7, np.uint64(2 ** 64 - 5), 0, 3]
    s = H.Voxel_Grid.directional_signed(h)
    assert s.dtype == np.int64 and s.shape == (2, 3, 4, 3) and s[1, 2, 3].tolist() == [-5, 0, 3]
    assert np.shares_memory(s, h)
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.set_receivers(np.zeros((3, 3)) + 1.0, np.ones(3) * 0.5)
    assert g._receive_shape(0, 10) == (3, 10, 1) and g._receive_shape(0, 10, True) == (3, 10, 1, 4)


# ---- the restatement by hand
def one_ray(o, d, c, r, n_bins=16, bin_len=1.0, frac=30):
    hist = np.zeros((1, n_bins, 1, 4), np.uint64)
    det = np.zeros((1, 2), np.uint64)
    receiver_step_dir([o], [d], np.array([np.inf]), np.zeros(1), np.ones((1, 1)), [c], [r], n_bins, bin_len, frac, hist, det)
    return hist, det


def test_two_rays_by_hand():
    # from the origin along +x through a receiver at (5, 0, 0): s = 5, bin 5; the sound travels towards +x, so it ARRIVES FROM -x: X < 0
    hist, det = one_ray([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [5.0, 0.0, 0.0], 0.5)
    want = np.zeros((1, 16, 1, 4), np.int64)
    want[0, 5, 0] = [2 ** 30, -(2 ** 30), 0, 0]
    assert np.array_equal(hist.view(np.int64), want) and det.tolist() == [[1, 0]]
    # direction (1, 2, 2): len = sqrt(9) = 3 exactly, s = (5 + 20 + 20) / 9 = 5
    hist, det = one_ray([0.0, 0.0, 0.0], [1.0, 2.0, 2.0], [5.0, 10.0, 10.0], 0.5)
    x = int(np.rint(2.0 ** 30 * -(1.0 / 3.0)))
    y = int(np.rint(2.0 ** 30 * -(2.0 / 3.0)))
    assert (x, y) == (-357913941, -715827883)
    want[0, 5, 0] = [2 ** 30, x, y, y]
    assert np.array_equal(hist.view(np.int64), want) and det.tolist() == [[1, 0]]
    # the opposite direction arrives from +x: X > 0 (the ambisonic sign convention)
    hist, _ = one_ray([10.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [5.0, 0.0, 0.0], 0.5)
    assert hist.view(np.int64)[0, 5, 0].tolist() == [2 ** 30, 2 ** 30, 0, 0]


def floor_and_ceiling():
    """tests/test_rain_api.py's room, restated: a floor triangle at z = 0 and a ceiling triangle at z = 10, both large: ray
    (0, 0, 1) + t (0, 0, -2) hits the floor at t = 0.5, X_Point (0, 0, 0)."""
    v = np.zeros((2, 4, 3))
    v[0, :3] = [(-10, -10, 0), (10, -10, 0), (0, 10, 0)]
    v[1, :3] = [(-10, -10, 10), (10, -10, 10), (0, 10, 10)]
    return v, np.array([3, 3], np.int32)


def test_one_rain_deposit_by_hand():
    v, nv = floor_and_ceiling()
    To = po.Topology(v, nv)
    part = po.VoxelGrid([To], domain=4)
    ray = np.array([[0.0, 0.0, 1.0, 0.0, 0.0, -2.0]])
    c, r = np.array([[0.0, 3.0, 4.0]]), np.array([0.5])
    sigma = np.ones((2, 1))
    n_bins, bin_len, frac = 16, 0.5, 40
    stats = {}
    hist, det, state, _ = receive_loop(po, To, part, ray, 2, c, r, n_bins, bin_len, frac, sigma=sigma, seed=5, rain=True, directional=True,
                                       stats=stats, nthreads=1)
    assert stats == {"eligible": 1, "occluded": 0} and det.tolist() == [[1, 0]]
    # v = (0, 3, 4), dist = 5, w = (4 / 5) * (0.25 / 25) = 0.008, bin (0.5 + 5 / 2) / 0.5 = 6 (tests/test_rain_api.py); the energy comes
    # from the receiver's side of the X_Point, so it arrives from -v / dist = (-0, -0.6, -0.8)
    m = ((1.0 * 1.0) * ((4.0 / 5.0) * (0.25 / 25.0))) * 2.0 ** 40
    w, y, z = int(np.rint(m)), int(np.rint(m * -(3.0 / 5.0))), int(np.rint(m * -(4.0 / 5.0)))
    assert (w, y, z) == (8796093022, -5277655813, -7036874418)
    want = np.zeros((1, n_bins, 1, 4), np.int64)
    want[0, 6, 0] = [w, 0, y, z]
    assert np.array_equal(hist.view(np.int64), want)
    omni, det0, state0, _ = receive_loop(po, To, part, ray, 2, c, r, n_bins, bin_len, frac, sigma=sigma, seed=5, rain=True, nthreads=1)
    assert np.array_equal(hist[..., 0], omni) and np.array_equal(det, det0) and state.tobytes() == state0.tobytes()


def test_channel_0_is_the_omni_restatement_and_the_signed_channels_are_bounded():
    m = H.scenes.shoebox()
    To = po.Topology(m.verts, m.nverts)
    o = po.VoxelGrid([To], domain=8)
    rays = H.scenes.burst_rays(3000, m.size)
    S = rays[0, :3]
    c = np.array([S + [1.0, 0.0, 0.0], [4.0, 3.5, 2.0], [7.0, 2.0, 1.5]])
    r = np.array([0.5, 0.6, 0.4])
    rng = np.random.default_rng(1)
    sigma, alpha = rng.uniform(0, 1, (To.P, 3)), rng.uniform(0, 0.5, (To.P, 3))
    casts, n_bins, bin_len, frac = 4, 200, 0.1, 30
    ev, _ = oracle_bounce_loop(po, To, o, rays, casts)
    omni = {"specular": replay_loop(po, To, rays, ev, c, r, n_bins, bin_len, frac, alpha=alpha),
            "scatter": receive_loop(po, To, o, rays, casts, c, r, n_bins, bin_len, frac, alpha=alpha, sigma=sigma, seed=3)[:3],
            "rain": receive_loop(po, To, o, rays, casts, c, r, n_bins, bin_len, frac, alpha=alpha, sigma=sigma, seed=3, rain=True)[:3]}
    for what, (h0, d0, s0) in omni.items():
        counts = np.zeros((3, n_bins), np.int64)
        h, d, s, _ = receive_loop(po, To, o, rays, casts, c, r, n_bins, bin_len, frac, alpha=alpha, sigma=None if what == "specular" else sigma,
                                  seed=3, rain=what == "rain", directional=True, counts=counts)
        assert h.shape == (3, n_bins, 3, 4) and h0.sum() > 0, what
        assert np.array_equal(h[..., 0], h0), what
        assert np.array_equal(d, d0) and s.tobytes() == s0.tobytes(), what
        assert counts.sum() == int(d[:, 0].sum()), what
        signed = H.Voxel_Grid.directional_signed(h)
        bound = h[..., 0].astype(np.int64) + counts[:, :, None]
        assert np.all(np.abs(signed) <= bound[..., None]), what
        assert np.any(signed != 0), what
    # receiver 0 sits at S + (1, 0, 0): its direct sound travels towards +x and arrives from -x
    first = np.flatnonzero(h[0, :, 0, 0])[0]
    assert H.Voxel_Grid.directional_signed(h)[0, first, 0, 0] < 0


# ---- argument checks that need no device
def test_the_bound_counts_the_four_channels(gpu_available):
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.set_receivers([[1.0, 1.0, 1.0]], [0.5])
    r = np.zeros((8, 6))
    h = np.zeros(64, np.uint64)                  # never written: the call is refused first
    d = np.zeros(2, np.uint64)
    base = 1 << 40

    def batch(flags, n_bins):
        return capi.lib.hare_receive_batch(g._h, g._kind, 0, 8, capi.ptr(r), None, None, 3, flags, n_bins, 0.01, 40, None, None, capi.ptr(h),
                                           capi.ptr(d), None)

    def dev(flags, n_bins):                      # addresses 8 GiB apart, never touched before the checks pass and a device is found
        return capi.lib.hare_receive_device(g._h, g._kind, 0, 8, base, None, None, 3, flags, n_bins, 0.01, 40, base + (8 << 30), base + (16 << 30),
                                            base + (24 << 30), base + (32 << 30), base + (40 << 30), None, None)
    n_bins = (1 << 25) + 1                       # 1 x n_bins x 1 <= 2^27 < 1 x n_bins x 1 x 4
    for call in (batch, dev):
        for flags in (capi.RECEIVE_DIRECTIONAL, capi.RECEIVE_DIRECTIONAL | capi.RECEIVE_DIFFUSE_RAIN):
            assert call(flags, n_bins) == capi.HARE_E_INVALID, call
            msg = capi.last_error()
            assert "receivers x n_bins x bands x 4" in msg and "2^27" in msg, msg
        assert call(capi.RECEIVE_DIRECTIONAL, (1 << 27) + 1) == capi.HARE_E_INVALID
    if not gpu_available:                        # the same call without the flag, and the largest directional one, pass that check
        assert dev(0, n_bins) == capi.HARE_E_NODEVICE
        assert dev(capi.RECEIVE_DIRECTIONAL, 1 << 25) == capi.HARE_E_NODEVICE


def test_device_call_holds_the_four_fold_histogram_to_the_overlap_check(gpu_available):
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.set_receivers([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0]], [0.5, 0.5])
    n, n_bins, base = 1000, 10, 1 << 40
    hist = base + (4 << 30)
    words = 2 * n_bins * 1                       # K x n_bins x B

    def rc(flags, det):
        return capi.lib.hare_receive_device(g._h, g._kind, 0, n, base, None, None, 4, flags, n_bins, 0.5, 30, base + (1 << 30), base + (2 << 30),
                                            base + (3 << 30), hist, det, None, None)
    # the detections start right behind an omni histogram: inside a directional one (addresses never touched)
    assert rc(capi.RECEIVE_DIRECTIONAL, hist + 8 * words) == capi.HARE_E_INVALID and "overlap" in capi.last_error()
    assert rc(capi.RECEIVE_DIRECTIONAL, hist + 8 * (4 * words - 1)) == capi.HARE_E_INVALID and "overlap" in capi.last_error()
    if not gpu_available:
        assert rc(0, hist + 8 * words) == capi.HARE_E_NODEVICE
        assert rc(capi.RECEIVE_DIRECTIONAL, hist + 8 * 4 * words) == capi.HARE_E_NODEVICE


def test_cpp_mirror_passes_the_flag(tmp_path, gpu_available):
    src = tmp_path / "d.cpp"
    src.write_text(r'''#include <cstdio>
#include "hare.hpp"
using namespace Hare::Geometry;
int main()
{
    // the cube [0,2]^3 as 12 triangles (bindings/cpp/receivers_example.cpp)
    const double c[8][3] = {{0, 0, 0}, {2, 0, 0}, {2, 2, 0}, {0, 2, 0}, {0, 0, 2}, {2, 0, 2}, {2, 2, 2}, {0, 2, 2}};
    const int f[12][3] = {{0, 1, 2}, {0, 2, 3}, {4, 6, 5}, {4, 7, 6}, {0, 5, 1}, {0, 4, 5}, {3, 2, 6}, {3, 6, 7}, {0, 3, 7}, {0, 7, 4}, {1, 5, 6}, {1, 6, 2}};
    std::vector<double> verts(12 * 12, 0.0);
    std::vector<int32_t> nverts(12, 3);
    for (int p = 0; p < 12; ++p)
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) verts[p * 12 + 3 * k + a] = c[f[p][k]][a];
    Topology t0(verts.data(), nverts.data(), 12);
    try {
        Voxel_Grid grid({&t0}, 4);
        grid.SetReceivers({1.5, 1.0, 1.0}, {0.25});
        // 64 rays from (0.5, 1, 1) along +x pass the receiver at s = 1: bin 2 of 0.5 m, E = 1 at 20 fractional bits
        std::vector<hare_ray> rays(64, hare_ray{0.5, 1.0, 1.0, 1.0, 0.0, 0.0});
        std::vector<uint64_t> hist, det;
        grid.Receive(rays, 0, 1, 8, 0.5, 20, hist, det, nullptr, nullptr, false, true);
        std::printf("directional ok %zu W %lld X %lld Y %lld Z %lld\n", hist.size(), (long long)hist[8], (long long)hist[9], (long long)hist[10],
                    (long long)hist[11]);
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 2;
    }
    return 0;
}
''')
    exe = str(tmp_path / "d")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "bindings", "cpp"),
                           str(src), "-L", os.path.join(ROOT, "hare_amd"), "-lhare_hip", "-Wl,-rpath," + os.path.join(ROOT, "hare_amd"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    if gpu_available:
        assert r.returncode == 0 and "directional ok 32 W 67108864 X -67108864 Y 0 Z 0" in r.stdout, r.stdout + r.stderr
    else:
        assert r.returncode == 2 and "no HIP device visible" in r.stdout, r.stdout + r.stderr
