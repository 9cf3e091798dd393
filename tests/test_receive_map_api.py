"""Receiver maps (include/hare_hip.h, "receivers", "Receiver maps") without a GPU: the exports are bound and declared; every refusal is
HARE_E_INVALID and changes nothing; K = 257 and K = 65 536 are accepted and read back; the options read as specified and set_receivers
after a map returns the scene to the linear loop; the grid the library built equals the numpy restatement's (tests/receive_map_ref.py).
The guarantee: over a seeded sweep inside the header's domain, no receiver that tests.receive_ref.receiver_step detects is missing from
the candidates.  Non-vacuity, from the restatement alone: every case of the device tests detects something, binned and unbinned, and in
the plane cases the mean share of receivers that are candidates is under one quarter."""
import struct

import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests.receive_cases import reference
from tests.receive_map_ref import MAX_K, build_grid, candidates, map_cases, map_layout
from tests.receive_ref import receiver_step

NEW = ("hare_scene_set_receiver_map", "hare_scene_get_receiver_map")
CASES = map_cases()


def grid():
    m = H.scenes.shoebox()
    T = H.Topology(m.verts, m.nverts)
    return H.Voxel_Grid([T], 8), T


def test_new_symbols_are_exported_bound_and_declared():
    hdr = open(capi.os.path.join(capi.os.path.dirname(capi._HERE), "include", "hare_hip.h")).read()
    for name in NEW:
        assert name in capi.SYMBOLS, name
        assert getattr(capi.lib, name).argtypes == capi.SYMBOLS[name][1]
        assert f"HARE_API int {name}(" in hdr, name


def map_options(g):
    return [g.get_option(o) for o in ("receivers", "receiver_map", "receiver_map_cells", "receiver_map_cell")]


def test_every_refusal_is_invalid_and_changes_nothing():
    g, T = grid()
    assert map_options(g) == [0, 0, 0, 0]
    one = ([[0.0, 0, 0]], [1.0])
    bad = [(np.zeros((0, 3)), np.zeros(0), 0.0), (np.zeros((MAX_K + 1, 3)), np.ones(MAX_K + 1), 0.0),
           ([[np.nan, 0, 0]], [1.0], 0.0), ([[0, -np.inf, 0]], [1.0], 0.0), ([[0, 0, 0]], [0.0], 0.0), ([[0, 0, 0]], [-1.0], 0.0),
           ([[0, 0, 0]], [np.inf], 0.0), ([[0, 0, 0]], [np.nan], 0.0), one + (np.nan,), one + (-1.0,), one + (np.inf,), one + (-np.inf,)]
    for when in ("empty", "map"):
        before = map_options(g)
        info = g.receiver_map_info() if when == "map" else None
        for centers, radii, cell in bad:
            with pytest.raises(H.HareError) as ei:
                g.set_receiver_map(centers, radii, cell)
            assert ei.value.code == capi.HARE_E_INVALID, (centers, radii, cell)
            assert map_options(g) == before
        if info is not None:
            now = g.receiver_map_info()
            assert all(np.array_equal(info[k], now[k]) for k in info)
        g.set_receiver_map(np.arange(30.0).reshape(10, 3), np.full(10, 0.5))
    with pytest.raises(H.HareError) as ei:
        H.Voxel_Grid([T], 8).receiver_map_info()
    assert ei.value.code == capi.HARE_E_STATE
    with pytest.raises(H.HareError) as ei:                     # the linear setter keeps its own limit
        g.set_receivers(np.zeros((257, 3)), np.ones(257))
    assert ei.value.code == capi.HARE_E_INVALID
    assert map_options(g)[:2] == [10, 1]


def rain_rc(g, flags):
    r, h, d = np.zeros((8, 6)), np.zeros(1 << 16, np.uint64), np.zeros(1 << 10, np.uint64)
    return capi.lib.hare_receive_batch(g._h, g._kind, 0, 8, capi.ptr(r), None, None, 2, flags, 4, 0.5, 30, None, None, capi.ptr(h), capi.ptr(d), None)


def test_rain_with_a_map_and_a_scattering_table_is_refused_before_anything_runs(gpu_available):
    g, T = grid()
    after = capi.HARE_OK if gpu_available else capi.HARE_E_NODEVICE
    g.set_receiver_map([[1.0, 1.0, 1.0]], [0.5])
    assert rain_rc(g, capi.RECEIVE_DIFFUSE_RAIN) == after                    # no table: the flag changes nothing, as without a map
    g.set_scattering(np.full((T.Polygon_Count, 2), 0.5))
    assert rain_rc(g, capi.RECEIVE_DIFFUSE_RAIN) == capi.HARE_E_INVALID
    assert rain_rc(g, capi.RECEIVE_DIFFUSE_RAIN | capi.RECEIVE_DIRECTIONAL) == capi.HARE_E_INVALID
    assert rain_rc(g, 0) == after
    g.set_receivers([[1.0, 1.0, 1.0]], [0.5])                                # the linear loop rains as before
    assert rain_rc(g, capi.RECEIVE_DIFFUSE_RAIN) == after


def same_grid(info, ref):
    assert np.array_equal(info["origin"], ref.origin) and info["cell"] == ref.h and info["pad"] == ref.R
    assert info["dims"].tolist() == ref.dims.tolist()
    assert np.array_equal(info["cell_start"], ref.cell_start) and np.array_equal(info["cell_items"], ref.cell_items)


@pytest.mark.parametrize("K", [257, MAX_K])
def test_more_than_256_receivers_are_accepted_and_read_back(K):
    g, _ = grid()
    rng = np.random.default_rng(K)
    centers, radii = rng.uniform(0.0, 10.0, (K, 3)), rng.uniform(0.05, 0.2, K)
    g.set_receiver_map(centers, radii)
    ref = build_grid(centers, radii)
    cell_bits = struct.unpack("<q", struct.pack("<d", ref.h))[0]
    assert map_options(g) == [K, 1, ref.cells, cell_bits]
    same_grid(g.receiver_map_info(), ref)
    assert sorted(g.receiver_map_info()["cell_items"].tolist()) == list(range(K))      # each receiver once
    g.set_receivers(centers[:3], radii[:3])
    assert map_options(g) == [3, 0, 0, 0]
    with pytest.raises(H.HareError) as ei:
        g.receiver_map_info()
    assert ei.value.code == capi.HARE_E_STATE


def test_the_plane_helper_lays_out_a_centred_lattice():
    c, r = H.Voxel_Grid.receiver_plane([0.0, 0.0], [10.0, 8.0], 1.2, 0.5, 0.2)
    assert c.shape == (21 * 17, 3) and (c[:, 2] == 1.2).all() and (r == 0.2).all()
    assert np.allclose([c[:, 0].min(), c[:, 0].max(), c[:, 1].min(), c[:, 1].max()], [0.0, 10.0, 0.0, 8.0])


GRID_SHAPES = [("plane", 1000), ("cell", 1000), ("cloud", 4096), ("coincident", 257), ("big", 300), ("onecell", 64), ("plane", 1), ("cloud", 2)]


@pytest.mark.parametrize("shape,K", GRID_SHAPES, ids=[f"{s}-{k}" for s, k in GRID_SHAPES])
def test_the_library_builds_the_reference_grid(shape, K):
    g, _ = grid()
    centers, radii, cell = map_layout(shape, K, H.scenes.shoebox().size, np.random.default_rng(K))
    g.set_receiver_map(centers, radii, cell)
    same_grid(g.receiver_map_info(), build_grid(centers, radii, cell))


def test_the_grid_at_its_edges():
    g, _ = grid()
    # the cell cap: the default cell and a caller's are doubled until the grid has at most 2^21 cells
    c = np.array([[0.0, 0, 0], [1000.0, 1000.0, 1000.0]])
    for cell in (0.0, 0.5, 3.0):
        g.set_receiver_map(c, [0.01, 0.01], cell)
        ref = build_grid(c, [0.01, 0.01], cell)
        assert ref.cells <= 1 << 21 and ref.h >= 1000.0 / 128
        same_grid(g.receiver_map_info(), ref)
    # an extent that overflows, radii from the smallest to the largest double: one cell, and still the reference's grid
    for c, r in [(np.array([[-1e308, 0, 0], [1e308, 0, 0]]), [1.0, 1.0]), (np.zeros((2, 3)), [5e-324, 1e308]), (np.zeros((1, 3)), [1e-320])]:
        g.set_receiver_map(c, r)
        ref = build_grid(c, r)
        info = g.receiver_map_info()
        assert np.array_equal(info["origin"], ref.origin) and info["dims"].tolist() == ref.dims.tolist()
        assert np.array_equal(np.array([info["cell"], info["pad"]]), np.array([ref.h, ref.R]), equal_nan=True)
        assert np.array_equal(info["cell_items"], ref.cell_items)


# ---- the guarantee
def sweep_rays(rng, m, centers, radii, lo, span):
    """m rays about the receivers: axis-parallel, diagonal, with zero components, starting inside a receiver, aimed at a receiver, and
    half-lines (t_end = +inf); directions scaled over sixty binary orders."""
    K = centers.shape[0]
    o = lo + rng.uniform(-0.3, 1.3, (m, 3)) * span
    d = rng.normal(size=(m, 3))
    kind = rng.integers(0, 6, m)
    ax = rng.integers(0, 3, m)
    for i in range(m):
        if kind[i] == 0:                                    # axis-parallel
            d[i] = 0.0
            d[i, ax[i]] = rng.choice([-1.0, 1.0])
        elif kind[i] == 1:                                  # diagonal: equal magnitudes (the major axis is a tie)
            d[i] = rng.choice([-1.0, 1.0], 3)
        elif kind[i] == 2:                                  # a zero component
            d[i, ax[i]] = 0.0
        elif kind[i] == 3:                                  # starting inside a receiver
            k = rng.integers(0, K)
            o[i] = centers[k] + rng.uniform(-0.5, 0.5, 3) * radii[k]
        elif kind[i] == 4:                                  # aimed to graze a receiver
            k = rng.integers(0, K)
            aim = centers[k] + rng.normal(size=3) * radii[k] * 0.7
            d[i] = aim - o[i]
    d = d * (2.0 ** rng.integers(-30, 31, (m, 1)))
    length = np.sqrt((d * d).sum(axis=1))
    reach = rng.uniform(0.0, 2.5, m) * np.linalg.norm(span) / np.where(length > 0, length, 1.0)
    t_end = np.where(rng.random(m) < 0.3, np.inf, reach)
    return o, d, t_end


def detected(o, d, t_end, centers, radii):
    """bool [m, K]: what tests.receive_ref.receiver_step detects, receiver by receiver (its counts per receiver, one ray at a time)."""
    m, K = o.shape[0], centers.shape[0]
    out = np.zeros((m, K), bool)
    for i in range(m):
        det = np.zeros((K, 2), np.uint64)
        receiver_step(o[i:i + 1], d[i:i + 1], t_end[i:i + 1], np.zeros(1), np.ones((1, 1)), centers, radii, 4, 1.0, 0, np.zeros((K, 4, 1), np.uint64), det)
        out[i] = det.sum(axis=1) > 0
    return out


SWEEP = [("plane", 400, 1.0), ("cell", 400, 1.0), ("cloud", 300, 1.0), ("coincident", 200, 1.0), ("big", 300, 1.0), ("onecell", 100, 1.0),
         ("cloud", 1, 1.0), ("plane", 300, 2.0 ** -20), ("cloud", 300, 2.0 ** 30)]


@pytest.mark.parametrize("shape,K,scale", SWEEP, ids=[f"{s}-{k}-{sc:g}" for s, k, sc in SWEEP])
def test_every_detected_receiver_is_a_candidate(shape, K, scale):
    rng = np.random.default_rng(4242 + K)
    size = np.array([10.0, 8.0, 4.0])
    centers, radii, cell = map_layout(shape, K, size, rng)
    centers, radii, cell = centers * scale, radii * scale, cell * scale          # the domain is in units of the cell: any size of room
    total = 0
    for placed in ("near", "edge"):
        g = build_grid(centers, radii, cell)
        lo, span = centers.min(axis=0), np.maximum(centers.max(axis=0) - centers.min(axis=0), 4 * radii.max())
        o, d, t_end = sweep_rays(rng, 160, centers, radii, lo, span)
        if placed == "edge":
            # coordinates up to the domain's edge: the scene shifted by just under 2^20 cells from the origin, rays starting as far
            # from the grid as the domain lets them and aimed back at it
            shift = np.array([0.999, -0.999, 0.999]) * (2.0 ** 20) * g.h - centers.max(axis=0) * np.array([1, 0, 1]) - centers.min(axis=0) * np.array([0, 1, 0])
            centers_s = centers + shift
            g = build_grid(centers_s, radii, cell)
            far = rng.random(160) < 0.5
            k = rng.integers(0, K, 160)
            o = o + shift
            o[far] = centers_s[k[far]] - np.sign(shift) * rng.uniform(0.2, 0.95, (int(far.sum()), 3)) * (2.0 ** 20) * g.h
            d[far] = (centers_s[k[far]] + rng.normal(size=(int(far.sum()), 3)) * radii[k[far], None] * 0.6) - o[far]
            t_end[far] = np.where(rng.random(int(far.sum())) < 0.5, np.inf, rng.uniform(0.9, 1.5, int(far.sum())))
            det = detected(o, d, t_end, centers_s, radii)
        else:
            det = detected(o, d, t_end, centers, radii)
        hit_end = o + d * np.where(np.isfinite(t_end), t_end, 0.0)[:, None]
        # inside the domain: within 2^20 cells of the grid's corner and of the origin
        assert (np.abs(o - g.origin) <= 2.0 ** 20 * g.h).all() and (np.abs(hit_end - g.origin) <= 2.0 ** 20 * g.h).all()
        assert (np.abs(o) <= 2.0 ** 20 * g.h).all() and (np.abs(g.origin + (g.dims * g.h)) <= 2.0 ** 20 * g.h * 1.001).all()
        cand = candidates(g, o, d, t_end)
        missing = det & ~cand
        assert not missing.any(), (shape, placed, np.argwhere(missing)[:4].tolist())
        total += int(det.sum())
    assert total > 20, total                                  # the sweep detects: the guarantee is not vacuous


def test_the_visit_rule_is_a_function_of_any_input():
    centers, radii, cell = map_layout("plane", 100, np.array([10.0, 8.0, 4.0]), np.random.default_rng(1))
    g = build_grid(centers, radii, cell)
    sp = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, 1e308, -1e308, 1.0, 2.0 ** -600])
    rng = np.random.default_rng(2)
    o, d = rng.choice(sp, (400, 3)), rng.choice(sp, (400, 3))
    t_end = rng.choice(np.array([np.inf, np.nan, 0.0, 1.0, 1e308, -1.0]), 400)
    cand = candidates(g, o, d, t_end)
    assert cand.shape == (400, 100)
    bad = ~np.isfinite(o).all(axis=1) | np.isnan(d).any(axis=1) | np.isnan(t_end)
    assert not cand[bad].any()                                # a NaN anywhere, or an infinite origin: no candidates


# ---- the device cases are not vacuous (the restatement alone)
@pytest.mark.parametrize("mc", CASES, ids=[c.name for c in CASES])
def test_device_case_detects_binned_and_unbinned(mc):
    want = reference(mc, keep=True)
    assert want["det"][:, 0].sum() > 0 and want["det"][:, 1].sum() > 0, mc.describe()
    assert want["hist"].any()
    if mc.map_shape in ("plane", "cell") and mc.K >= 256:
        pairs = np.array(want["share"], np.float64)
        assert pairs[:, 0].sum() / pairs[:, 1].sum() < 0.25, mc.describe()
