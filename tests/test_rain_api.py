"""Diffuse rain (include/hare_hip.h, "receivers", "Diffuse rain") without a GPU: the flag's value is a bit of its own and every binding
repeats it; the enlarged work array of hare_receive_device is what the header's formula says and what the overlap check holds a caller
to; the numpy restatement the GPU tests compare against (tests/receive_ref.py) gives the hand-worked answer on one ray over a floor, and
without rain it is the scattering loop."""
import os
import re
import subprocess

import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from oracle import pyoracle as po
from tests.receive_ref import receive_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hare_hip.h")


def header_defines():
    return {k: int(v) for k, v in re.findall(r"#define\s+(HARE_[A-Z_]+)\s+(\d+)u", open(HEADER).read())}


def test_flag_is_a_bit_of_its_own_and_bound_everywhere():
    d = header_defines()
    rain = d["HARE_RECEIVE_DIFFUSE_RAIN"]
    assert rain == 128 == capi.RECEIVE_DIFFUSE_RAIN and rain & (rain - 1) == 0
    shoot = [v for k, v in d.items() if k.startswith("HARE_SHOOT_")]
    assert len(shoot) >= 7 and all(v & rain == 0 for v in shoot)
    assert rain & (0xF000 | 0x40000 | 0x80000) == 0                 # the developer bits and the internal ones (launch.cpp asserts it too)
    launch = open(os.path.join(ROOT, "hare_amd", "csrc", "launch.cpp")).read()
    assert "static_assert((HARE_RECEIVE_DIFFUSE_RAIN &" in launch
    cs = open(os.path.join(ROOT, "bindings", "csharp", "HareHip.cs")).read()
    assert re.search(r"HARE_RECEIVE_DIFFUSE_RAIN\s*=\s*128\s*;", cs)
    part = open(os.path.join(ROOT, "bindings", "csharp", "Gpu_Spatial_Partition.cs")).read()
    assert re.search(r"public long Receive\([^)]*bool state_in, bool rain\)", part)
    assert "rain ? HareHip.HARE_RECEIVE_DIFFUSE_RAIN : 0u" in part
    for fn in (H.Voxel_Grid.Receive_batch, H.Voxel_Grid.Receive_batch_sharded, H.Voxel_Grid.receive_device):
        assert "rain" in fn.__code__.co_varnames[:fn.__code__.co_argcount], fn


def test_work_size_formula(tmp_path):
    src = tmp_path / "w.c"
    src.write_text('#include "hare_hip.h"\n#include <stdio.h>\nint main(void){long long n[] = {0, 1, 4097, 65537, 1LL << 31};\n'
                   'for (int k = 0; k < 5; ++k)\n    printf("%lld\\n", (long long)HARE_RECEIVE_RAIN_WORK_BYTES(n[k]));\nreturn 0;}\n')
    exe = str(tmp_path / "w")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    ns = [0, 1, 4097, 65537, 1 << 31]
    assert got == [H.Voxel_Grid.receive_work_bytes(n, rain=True) for n in ns] == [80 * n + 256 for n in ns]
    assert H.Voxel_Grid.receive_work_bytes(4097) == 8 * 4097
    # the scratch the library carves out of it: 8 n bytes of the loop, up to 15 of alignment, 48 + 8 + 3 x 4 = 68 n of rain
    assert all(8 * n + 15 + 68 * n <= 80 * n + 256 for n in ns)


def test_device_call_holds_the_enlarged_work_array_to_the_overlap_check():
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.set_receivers([[1.0, 1.0, 1.0]], [0.5])
    n, base = 1000, 1 << 40
    work = base + (2 << 30)
    # the events start 8 n + 64 bytes behind the work array: clear of its 2 n int32, inside its rain scratch (addresses never touched)
    rc = capi.lib.hare_receive_device(g._h, g._kind, 0, n, base, None, None, 4, capi.RECEIVE_DIFFUSE_RAIN, 10, 0.5, 30, base + (1 << 30), work,
                                      work + 8 * n + 64, base + (4 << 30), base + (5 << 30), None, None)
    assert rc == capi.HARE_E_INVALID and "overlap" in capi.last_error()


def test_cpp_mirror_passes_the_flag(tmp_path, gpu_available):
    src = tmp_path / "r.cpp"
    src.write_text(r'''#include <cstdio>
#include "hare.hpp"
using namespace Hare::Geometry;
int main()
{
    // the cube [0,2]^3 as 12 triangles (bindings/cpp/receivers_example.cpp), every face scattering half its energy
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
        grid.SetReceivers({1.5, 1.5, 1.5}, {0.25});
        grid.SetScattering(0, 1, std::vector<double>(12, 0.5));
        std::vector<hare_ray> rays(64, hare_ray{0.5, 0.6, 0.7, 0.3, -1.0, 0.2});
        std::vector<uint64_t> hist, det;
        grid.Receive(rays, 0, 3, 8, 0.5, 20, hist, det, nullptr, nullptr, true);
        std::printf("rain ok %zu\n", hist.size());
    } catch (const std::exception& e) {
        std::printf("%s\n", e.what());
        return 2;
    }
    return 0;
}
''')
    exe = str(tmp_path / "r")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "bindings", "cpp"),
                           str(src), "-L", os.path.join(ROOT, "hare_amd"), "-lhare_hip", "-Wl,-rpath," + os.path.join(ROOT, "hare_amd"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    if gpu_available:
        assert r.returncode == 0 and "rain ok 8" in r.stdout, r.stdout + r.stderr
    else:
        assert r.returncode == 2 and "no HIP device visible" in r.stdout, r.stdout + r.stderr


# ---- the restatement on a hand-worked case
def floor_and_ceiling():
    """A floor triangle at z = 0 and a ceiling triangle at z = 10, both large: ray (0, 0, 1) + t (0, 0, -2) hits the floor at t = 0.5,
    X_Point (0, 0, 0)."""
    v = np.zeros((2, 4, 3))
    v[0, :3] = [(-10, -10, 0), (10, -10, 0), (0, 10, 0)]
    v[1, :3] = [(-10, -10, 10), (10, -10, 10), (0, 10, 10)]
    return v, np.array([3, 3], np.int32)


def test_rain_of_one_ray_over_a_floor_by_hand():
    v, nv = floor_and_ceiling()
    To = po.Topology(v, nv)
    part = po.VoxelGrid([To], domain=4)
    ray = np.array([[0.0, 0.0, 1.0, 0.0, 0.0, -2.0]])
    c, r = np.array([[0.0, 3.0, 4.0]]), np.array([0.5])
    sigma = np.ones((2, 1))
    n_bins, bin_len, frac = 16, 0.5, 40
    # the shadow ray (0, 0, 0) -> (0, 3, 4) meets the ceiling, but at t = 2.5: beyond t_max = 1, so the receiver is seen
    ev, _ = part.shoot(np.array([[0.0, 0.0, 0.0, 0.0, 3.0, 4.0]]), excl1=np.array([0], np.int32))
    assert ev["hit"][0] == 1 and ev["poly_id"][0] == 1 and ev["t"][0] == 2.5
    stats = {}
    hist, det, state, _ = receive_loop(po, To, part, ray, 2, c, r, n_bins, bin_len, frac, sigma=sigma, seed=5, rain=True, stats=stats, nthreads=1)
    # v = (0, 3, 4), d2 = 25, n' = (0, 0, 1) (the ray came from above), cs = 4: eligible (25 > 0.25, 4 > 0) and not occluded
    w = (4.0 / 5.0) * (0.25 / 25.0)                                    # cos / dist * r^2 / d2: 0.008
    assert abs(w - 0.008) < 1e-17
    x = (0.5 + 5.0 / 2.0) / 0.5                                        # L' = 0 + 0.5, dist / len = 5 / 2: bin 6
    q = int(np.rint(((1.0 * 1.0) * w) * 2.0 ** 40))
    assert stats == {"eligible": 1, "occluded": 0}
    want = np.zeros((1, n_bins, 1), np.uint64)
    want[0, int(x), 0] = q
    # cast 0 passes the receiver behind its origin (s < 0) and cast 1, the diffuse segment (sigma = 1), is suppressed: the rain is all
    assert np.array_equal(hist, want) and det.tolist() == [[1, 0]]
    assert x == 6.0 and q == 8796093022
    # the state is the scattered one: L = 0.5 + t of cast 1, E = 1 (weight sigma / p = 1)
    _, _, state_plain, _ = receive_loop(po, To, part, ray, 2, c, r, n_bins, bin_len, frac, sigma=sigma, seed=5, rain=False, nthreads=1)
    assert state.tobytes() == state_plain.tobytes() and state[1, 0] == 1.0
    # a receiver behind the floor's plane (cs < 0) or one the point is inside (d2 <= r^2) gets nothing
    for cc in ([[0.0, 3.0, -4.0]], [[0.0, 0.3, 0.1]]):
        s2 = {}
        receive_loop(po, To, part, ray, 2, np.array(cc), r, n_bins, bin_len, frac, sigma=sigma, seed=5, rain=True, stats=s2, nthreads=1)
        assert s2 == {}, cc


def test_restatement_without_rain_is_the_scatter_loop():
    m = H.scenes.shoebox()
    To = po.Topology(m.verts, m.nverts)
    o = po.VoxelGrid([To], domain=8)
    rays = H.scenes.burst_rays(2000, m.size)
    c, r = np.array([[4.0, 3.5, 2.0], [7.0, 2.0, 1.5]]), np.array([0.6, 0.4])
    rng = np.random.default_rng(1)
    sigma, alpha = rng.uniform(0, 1, (To.P, 3)), rng.uniform(0, 0.5, (To.P, 3))
    a = receive_loop(po, To, o, rays, 4, c, r, 200, 0.1, 30, alpha=alpha, sigma=sigma, seed=3)
    b = receive_loop(po, To, o, rays, 4, c, r, 200, 0.1, 30, alpha=alpha, sigma=sigma, seed=3, rain=False)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    # with rain: the same state, another histogram
    stats = {}
    h, d, s, _ = receive_loop(po, To, o, rays, 4, c, r, 200, 0.1, 30, alpha=alpha, sigma=sigma, seed=3, rain=True, stats=stats)
    assert s.tobytes() == a[2].tobytes() and not np.array_equal(h, a[0]) and stats["eligible"] > 1000 and stats["occluded"] == 0
