"""Diffuse scattering in the receive loop (include/hare_hip.h, "receivers", "Scattering") without a GPU: the new export is bound and
declared, hare_scene_set_scattering validates as hare_scene_set_absorption does plus the shared-B rule, removes a table, and the bands and
"scatter_seed" read back; the numpy restatement the GPU tests compare against (tests/scatter_ref.py) draws SplitMix64's numbers, and its
sampler keeps to the half-space, the ray's length, the cosine law and unbiased band weights; the C++ example refuses bad input."""
import os
import subprocess

import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests import scatter_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (1 << 64) - 1


def grid(topologies=1):
    m = H.scenes.shoebox()
    Ts = [H.Topology(m.verts, m.nverts) for _ in range(topologies)]
    return H.Voxel_Grid(Ts, 8), Ts[0]


def invalid(fn, *args):
    with pytest.raises(H.HareError) as ei:
        fn(*args)
    assert ei.value.code == capi.HARE_E_INVALID


def test_new_symbol_is_exported_bound_and_declared():
    hdr = open(os.path.join(ROOT, "include", "hare_hip.h")).read()
    name = "hare_scene_set_scattering"
    assert name in capi.SYMBOLS
    assert getattr(capi.lib, name).argtypes == capi.SYMBOLS[name][1]
    assert f"HARE_API int {name}(" in hdr
    assert hasattr(H.Voxel_Grid, "set_scattering")


def test_scattering_setter_validates():
    g, T = grid(2)
    P = T.Polygon_Count
    for top, sigma in [(2, np.zeros((P, 2))), (-1, np.zeros((P, 2))), (0, np.zeros((P, 9))), (0, np.full((P, 2), -0.01)),
                       (0, np.full((P, 2), 1.01)), (0, np.full((P, 2), np.nan)), (0, np.full((P, 2), np.inf))]:
        invalid(g.set_scattering, sigma, top)
    assert capi.lib.hare_scene_set_scattering(g._h, 0, 0, capi.ptr(np.zeros(P))) == capi.HARE_E_INVALID     # B = 0 with a table
    assert capi.lib.hare_scene_set_scattering(g._h, 0, -1, None) == capi.HARE_E_INVALID
    assert capi.lib.hare_scene_set_scattering(g._h, 0, 2, None) == capi.HARE_E_INVALID                    # null table
    assert capi.lib.hare_scene_set_scattering(None, 0, 2, capi.ptr(np.zeros((P, 2)))) == capi.HARE_E_INVALID
    one = np.zeros((P, 2))
    one[3, 1] = np.nan
    invalid(g.set_scattering, one)                                   # a single bad value anywhere
    assert g.get_option("bands:0") == 1 and g.get_option("bands:1") == 1     # a refused call changes nothing


def test_bands_are_shared_with_absorption_in_both_orders_and_removal():
    g, T = grid(2)
    P = T.Polygon_Count
    # scattering alone fixes B
    g.set_scattering(np.full((P, 3), 0.5))
    assert g.get_option("bands") == 3 and g.get_option("bands:0") == 3 and g.get_option("bands:1") == 1
    invalid(g.set_absorption, np.zeros((P, 4)))                      # absorption must match it
    g.set_absorption(np.zeros((P, 3)))
    g.set_scattering(np.full((P, 3), 0.25))                          # replacing with the same B
    invalid(g.set_scattering, np.zeros((P, 5)))                      # ... but not another one while absorption is set
    assert g.get_option("bands:0") == 3
    g.set_scattering(None)                                           # removal: the absorption table keeps B
    assert g.get_option("bands:0") == 3
    g.set_absorption(np.zeros((P, 6)))                               # absorption alone: replaced with another B, as before
    assert g.get_option("bands:0") == 6
    # absorption first fixes B for scattering
    g.set_absorption(np.zeros((P, 2)), 1)
    invalid(g.set_scattering, np.zeros((P, 8)), 1)
    g.set_scattering(np.full((P, 2), 1.0), 1)
    assert g.get_option("bands:1") == 2
    # a topology with scattering only: removal returns it to B = 1
    h, _ = grid()
    h.set_scattering(np.zeros((P, 8)))
    assert h.get_option("bands") == 8
    h.set_scattering(np.zeros((P, 5)))                               # no absorption table: scattering alone may change B
    assert h.get_option("bands") == 5
    h.set_scattering(None)
    assert h.get_option("bands") == 1
    h.set_scattering(None)                                           # removing nothing is fine
    assert capi.lib.hare_scene_set_scattering(h._h, 1, 0, None) == capi.HARE_E_INVALID       # ... but not on a topology it lacks


def test_scatter_seed_round_trips_as_int64():
    g, _ = grid()
    assert g.get_option("scatter_seed") == 0
    for v in (1, -1, -(1 << 63), (1 << 63) - 1, 0x0123456789ABCDEF, -12345):
        g.set_option("scatter_seed", v)
        assert g.get_option("scatter_seed") == v


def splitmix64(seed, k):
    """The first k outputs of SplitMix64 (Steele, Lea, Flood 2014), in Python integers."""
    out, s = [], seed & MASK
    for _ in range(k):
        s = (s + 0x9E3779B97F4A7C15) & MASK
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        out.append(z ^ (z >> 31))
    return out


def test_rng_is_splitmix64():
    assert int(sr.mix(np.array([sr.G]))[0]) == 0xE220A8397B1DCDAF        # SplitMix64 seeded with 0: its first output
    for seed in (0, 1, 0xDEADBEEF, MASK):
        want = splitmix64(seed, 6)
        states = np.array([(seed + (i + 1) * 0x9E3779B97F4A7C15) & MASK for i in range(6)], np.uint64)
        assert [int(v) for v in sr.mix(states)] == want
    # base and u_j against Python integers
    for seed, g, c, j in ((0, 0, 0, 0), (-1, 12345, 7, 64), (1 << 62, 4096, 4095, 255), (-(1 << 63), 65536, 3, 1)):
        S = seed & MASK
        base = splitmix64(((splitmix64(S, 1)[0] ^ g) - 0x9E3779B97F4A7C15) & MASK, 1)[0]     # mix(x) = first output seeded with x - G
        assert int(sr.ray_base(seed, np.array([g], np.uint64))[0]) == base
        word = ((c << 8) | j) * 0x9E3779B97F4A7C15
        z = splitmix64((base + word - 0x9E3779B97F4A7C15) & MASK, 1)[0]
        u = sr.uniform(np.array([base], np.uint64), c, j)[0]
        assert u == (z >> 11) * 2.0 ** -53 and 0.0 <= u < 1.0


N = 1 << 20


@pytest.fixture(scope="module")
def draws():
    """~10^6 diffuse draws: random unit normals and incoming directions of random length, the header's RNG for cast 3."""
    rng = np.random.default_rng(11)
    n = rng.normal(size=(N, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    n[:16] = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 1, 0], [1, 0, -0.0], [-1, 0, 0], [0, -1, 0], [0.6, 0, -0.8]] * 2
    d = rng.normal(size=(N, 3)) * rng.uniform(0.1, 40.0, (N, 1))
    base = sr.ray_base(-3, np.arange(N, dtype=np.uint64))
    x, y, r2 = sr.disc(base, 3)
    out, nprime = sr.direction(d, n, x, y, r2)
    return d, n, out, nprime, base


def test_diffuse_directions_point_away_from_the_surface_the_ray_hit(draws):
    d, n, out, nprime, _ = draws
    dot_in = (d * n).sum(1)
    assert np.all(np.where(dot_in[:, None] > 0, -n, n) == nprime)     # n' faces the side the ray came from
    assert np.all((out * nprime).sum(1) >= 0)
    assert np.all((d * nprime).sum(1) <= 0)


def test_diffuse_directions_keep_the_incoming_length(draws):
    d, _, out, _, _ = draws
    ld, lo = np.linalg.norm(d, axis=1), np.linalg.norm(out, axis=1)
    assert np.max(np.abs(lo - ld) / ld) < 8 * np.finfo(np.float64).eps


def test_diffuse_directions_follow_the_cosine_law(draws):
    _, _, out, nprime, _ = draws
    cos = (out * nprime).sum(1) / np.linalg.norm(out, axis=1)
    assert abs(cos.mean() - 2.0 / 3.0) < 0.005                        # E[cos] under p(w) = cos / pi
    assert abs((cos * cos).mean() - 0.5) < 0.005                      # E[cos^2]


def test_band_weights_are_unbiased_for_an_uneven_row(draws):
    base = draws[4]
    row = np.array([0.0, 0.05, 0.2, 0.5, 0.7, 0.9, 1.0, 0.35])
    u0 = sr.uniform(base, 2, 0)
    p, diffuse = sr.choose(np.broadcast_to(row, (N, 8)), u0)
    assert abs(diffuse.mean() - row.mean()) < 0.005
    w = sr.weights(np.broadcast_to(row, (N, 8)), p, diffuse)
    assert np.all(np.isfinite(w))
    assert np.all(np.abs(w.mean(0) - 1.0) < 0.01), w.mean(0)
    # p = 0 and p = 1: every weight exactly 1
    for r in (np.zeros(8), np.ones(8)):
        p, dif = sr.choose(np.broadcast_to(r, (1000, 8)), u0[:1000])
        assert np.all(dif == (r[0] == 1.0)) and np.all(sr.weights(np.broadcast_to(r, (1000, 8)), p, dif) == 1.0)


def test_rejection_fallback_leaves_along_the_normal():
    rng = np.random.default_rng(5)
    n = rng.normal(size=(64, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    d = rng.normal(size=(64, 3)) * 3.0
    z = np.zeros(64)
    out, nprime = sr.direction(d, n, z, z, z)
    ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    assert np.array_equal(out, nprime * ln[:, None])


def test_rejection_loop_takes_about_1_27_tries(draws):
    base = draws[4][:100000]
    tries = np.full(base.shape[0], sr.TRIES)
    for t in range(sr.TRIES - 1, -1, -1):
        x = 2.0 * sr.uniform(base, 3, 1 + 2 * t) - 1.0
        y = 2.0 * sr.uniform(base, 3, 2 + 2 * t) - 1.0
        tries = np.where(x * x + y * y < 1.0, t + 1, tries)
    assert abs(tries.mean() - 4.0 / np.pi) < 0.01


def test_cpp_scattering_example_refuses_bad_input(tmp_path, gpu_available):
    exe = str(tmp_path / "hare_scattering")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "bindings", "cpp"), os.path.join(ROOT, "bindings", "cpp", "scattering_example.cpp"),
                           "-L", os.path.join(ROOT, "hare_amd"), "-lhare_hip", "-Wl,-rpath," + os.path.join(ROOT, "hare_amd"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert "bands 8, scatter_seed -7" in r.stdout, r.stdout + r.stderr
    assert "refused 4" in r.stdout
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device visible" in r.stdout and "receive:" not in r.stdout
    else:
        assert r.returncode == 0 and "same seed equal, other seed differs, receiver 1 nonzero yes" in r.stdout, r.stdout
