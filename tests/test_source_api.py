"""The point source on the CPU (include/hare_hip.h, "receivers", "Source"): hare_scene_set_source's refusals, the options it adds, the
order of the checks of hare_emit_device and hare_receive_source (HARE_E_INVALID before HARE_E_NODEVICE before HARE_E_STATE), and the
properties of the definition itself as tests/source_ref.py restates it: unit directions, no drift, no exhausted rejection, the chunk
identity.  And that the device cases of tests/test_gpu_source.py reach every path of the directivity lookup."""
import ctypes as C

import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests import source_ref as sr

E_INVALID, E_NODEVICE, E_STATE = capi.HARE_E_INVALID, capi.HARE_E_NODEVICE, capi.HARE_E_STATE


def grid():
    m = H.scenes.shoebox()
    return H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8), m


def code(call):
    with pytest.raises(H.HareError) as ei:
        call()
    return ei.value.code


def test_setter_refusals():
    g, _ = grid()
    ok = dict(pos=(1.0, 2.0, 3.0), power=np.ones(3), frame=np.eye(3), gain=np.ones((6, 2, 2, 3)))
    g.set_source(**ok)
    bad = np.ones((6, 2, 2, 3))
    for value in (np.nan, np.inf, -1e-300):
        bad_gain = bad.copy()
        bad_gain[5, 1, 1, 2] = value
        assert code(lambda: g.set_source(**dict(ok, gain=bad_gain))) == E_INVALID
        assert code(lambda: g.set_source(**dict(ok, power=(1.0, value, 1.0)))) == E_INVALID
    for value in (np.nan, np.inf, -np.inf):
        assert code(lambda: g.set_source(**dict(ok, pos=(0.0, value, 0.0)))) == E_INVALID
        f = np.eye(3)
        f[2, 1] = value
        assert code(lambda: g.set_source(**dict(ok, frame=f))) == E_INVALID
    lib, p3, one = capi.lib, np.zeros(3), np.ones(6 * 65 * 65 * 9)
    for B in (0, 9, -1):
        assert lib.hare_scene_set_source(g._h, p3.ctypes.data, B, None, None, 0, None) == E_INVALID
    for R in (-1, 65):
        assert lib.hare_scene_set_source(g._h, p3.ctypes.data, 1, None, None, R, one.ctypes.data) == E_INVALID
    assert lib.hare_scene_set_source(g._h, p3.ctypes.data, 1, None, None, 0, one.ctypes.data) == E_INVALID          # a table with R = 0
    assert lib.hare_scene_set_source(g._h, p3.ctypes.data, 1, None, None, 4, None) == E_INVALID                      # R without a table
    assert lib.hare_scene_set_source(g._h, None, 1, None, None, 0, None) == E_INVALID
    assert lib.hare_scene_set_source(None, p3.ctypes.data, 1, None, None, 0, None) == E_INVALID
    assert "hare_scene_set_source" in capi.last_error() or "null scene" in capi.last_error()
    # a refused call leaves the source as it was
    assert (g.get_option("source"), g.get_option("source_bands"), g.get_option("source_res")) == (1, 3, 2)
    # the limits themselves pass
    assert lib.hare_scene_set_source(g._h, p3.ctypes.data, 8, None, None, 64, np.zeros(6 * 64 * 64 * 8).ctypes.data) == capi.HARE_OK
    assert (g.get_option("source_bands"), g.get_option("source_res")) == (8, 64)
    with pytest.raises(ValueError):
        g.set_source((0, 0, 0), power=np.ones(2), gain=np.ones((6, 2, 2, 3)))
    with pytest.raises(ValueError):
        g.set_source((0, 0, 0), gain=np.ones((6, 2, 3, 1)))


def test_options_round_trip():
    g, _ = grid()
    assert (g.get_option("source"), g.get_option("source_bands"), g.get_option("source_res"), g.get_option("source_seed")) == (0, 0, 0, 0)
    for seed in (0, -7, 12345, -2 ** 63, 2 ** 63 - 1):
        assert g.set_option("source_seed", seed).get_option("source_seed") == seed
    assert g.get_option("scatter_seed") == 0                       # a seed of its own
    g.set_source((0.5, 0.5, 0.5))
    assert (g.get_option("source"), g.get_option("source_bands"), g.get_option("source_res")) == (1, 1, 0)
    g.set_source((0.5, 0.5, 0.5), power=np.ones(5), gain=np.ones((6, 16, 16, 5)))
    assert (g.get_option("source"), g.get_option("source_bands"), g.get_option("source_res")) == (1, 5, 16)
    g.set_source((0.5, 0.5, 0.5), power=np.ones(2))               # replaced by a source without a table
    assert (g.get_option("source_bands"), g.get_option("source_res")) == (2, 0)
    for name in ("source", "source_bands", "source_res"):          # read-only figures
        assert code(lambda: g.set_option(name, 1)) == E_INVALID


def test_emit_device_checks_in_order(gpu_available):
    g, _ = grid()
    lib, h = capi.lib, g._h
    emit = lambda n, first, rays, state: lib.hare_emit_device(h, n, first, rays, state, None)
    # 1. ranges, before the buffers are looked at
    for n, first in ((-1, 0), (2 ** 31 - 255, 0), (4, -1), (4, 2 ** 62 - 3), (0, 2 ** 62 + 1)):
        assert emit(n, first, None, None) == E_INVALID, (n, first)
    # 2. null and overlapping buffers (addresses are only compared: nothing is dereferenced before a device is found)
    assert emit(4, 0, None, 4096) == E_INVALID and emit(4, 0, 4096, None) == E_INVALID
    assert emit(4, 0, 4096, 4096 + 4 * 48 - 8) == E_INVALID and emit(4, 0, 4096 + 4 * 16 - 8, 4096) == E_INVALID
    if gpu_available:
        # 3. passed; 4. no source
        assert emit(0, 0, None, None) == E_STATE and "no source" in capi.last_error()
        g.set_source((0, 0, 0))
        assert emit(0, 0, None, None) == capi.HARE_OK and emit(0, 2 ** 62, None, None) == capi.HARE_OK
    else:
        assert emit(4, 0, 4096, 1 << 20) == E_NODEVICE          # before "no source"
        g.set_source((0, 0, 0))
        assert emit(4, 2 ** 62 - 4, 4096, 1 << 20) == E_NODEVICE
    # the state's size follows the source's bands: (1 + 8) planes now reach the rays
    g.set_source((0, 0, 0), power=np.ones(8))
    assert emit(4, 0, 4096 + 4 * 16, 4096) == E_INVALID


def test_receive_source_checks_in_order(gpu_available):
    g, m = grid()
    SP = H.Spatial_Partition
    assert code(lambda: g.Receive_source(16, 2, 10, 0.1, first_ray=-1)) == E_INVALID
    assert code(lambda: g.Receive_source(16, 2, 10, 0.1, first_ray=2 ** 62 - 15)) == E_INVALID
    assert code(lambda: g.Receive_source(16, 0, 10, 0.1)) == E_INVALID              # hare_receive_batch's own checks
    assert code(lambda: g.Receive_source(16, 2, 10, 0.0)) == E_INVALID
    # no receivers, no source: a matter of state, found behind the device checks
    assert code(lambda: g.Receive_source(16, 2, 10, 0.1)) == (E_STATE if gpu_available else E_NODEVICE)
    g.set_receivers([np.asarray(m.size) * 0.5], [0.5])
    assert code(lambda: g.Receive_source(16, 2, 10, 0.1)) == (E_STATE if gpu_available else E_NODEVICE)
    if gpu_available:
        assert "no source" in capi.last_error()
    # the source's bands against the topology's: refused before any device is looked for
    g.set_source(np.asarray(m.size) * 0.3, power=np.ones(3))
    assert code(lambda: g.Receive_source(16, 2, 10, 0.1)) == E_INVALID and "bands" in capi.last_error()
    g.set_absorption(np.full((g.Model[0].Polygon_Count, 3), 0.1))
    if not gpu_available:
        assert code(lambda: g.Receive_source(16, 2, 10, 0.1)) == E_NODEVICE
    # the sharded call refuses scenes whose source or seed differ
    g2, _ = grid()
    g2.set_receivers([np.asarray(m.size) * 0.5], [0.5]).set_absorption(np.full((g.Model[0].Polygon_Count, 3), 0.1))
    both = lambda: SP.Receive_source_sharded([g, g2], 16, 2, 10, 0.1)
    assert code(both) == E_INVALID and "source" in capi.last_error()                # g2 has none
    g2.set_source(np.asarray(m.size) * 0.3, power=(1.0, 1.0, 0.5))
    assert code(both) == E_INVALID
    g2.set_source(np.asarray(m.size) * 0.3, power=np.ones(3)).set_option("source_seed", 1)
    assert code(both) == E_INVALID
    g2.set_option("source_seed", 0)
    if not gpu_available:
        assert code(both) == E_NODEVICE


# ---- the definition, as tests/source_ref.py restates it
PROPERTY_CASES = [(n, seed, first) for n in (65536, 4097) for seed in (0, -7, 12345) for first in (0, 2 ** 32 - 100, 2 ** 40)]


@pytest.fixture(scope="module")
def property_directions():
    return {c: sr.directions(c[1], c[2], c[0]) for c in PROPERTY_CASES}


def test_directions_are_unit_vectors_without_drift(property_directions):
    """|d| = 1 within 4 ulp (2^-52 each: the three products, two sums and the sqrt round once each).  Each mean component of n
    independent uniform directions has variance 1 / (3 n): within 4 sigma (the seeds are fixed; a true 4-sigma event is 6e-5)."""
    for (n, seed, first), (d, _) in property_directions.items():
        norm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        assert np.abs(norm - 1.0).max() <= 4 * 2.0 ** -52, (n, seed, first)
        sigma = 1.0 / np.sqrt(3.0 * n)
        assert np.abs(d.mean(axis=0)).max() <= 4 * sigma, (n, seed, first, d.mean(axis=0) / sigma)


def test_directions_cover_the_cube_faces_evenly(property_directions):
    """A third of the sphere lies over each pair of opposite cube faces: the share p = 1/3 of n rays has sigma sqrt(p (1 - p) / n)."""
    for (n, seed, first), (d, _) in property_directions.items():
        lead = np.abs(d).argmax(axis=1)
        sigma = np.sqrt((1.0 / 3.0) * (2.0 / 3.0) / n)
        for f in range(3):
            assert abs(np.count_nonzero(lead == f) / n - 1.0 / 3.0) <= 4 * sigma, (n, seed, first, f)


def test_the_rejection_never_runs_out():
    for n, seed, first in PROPERTY_CASES:
        assert not sr.exhausted(seed, first, n).any(), (n, seed, first)


def test_chunk_identity():
    g = sr.table(2, 3)
    for seed, a, n, k in ((0, 0, 4097, 1500), (-7, 2 ** 32 - 100, 4097, 100), (12345, 2 ** 40, 513, 512), (5, 7, 300, 0)):
        whole = sr.emit(seed, a, n, sr.POS, sr.powers(3), sr.FRAMES["rotation"], 2, g)
        tail = sr.emit(seed, a + k, n - k, sr.POS, sr.powers(3), sr.FRAMES["rotation"], 2, g)
        assert whole[0][k:].tobytes() == tail[0].tobytes() and np.ascontiguousarray(whole[1][:, k:]).tobytes() == tail[1].tobytes()
    # another seed, other rays; the scattering RNG's words are not the source's (another counter)
    assert sr.directions(0, 0, 64)[0].tobytes() != sr.directions(1, 0, 64)[0].tobytes()


def test_emit_without_a_table_is_the_power():
    rays, state = sr.emit(3, 10, 257, sr.POS, sr.powers(8), None, 0, None)
    assert np.array_equal(rays[:, :3], np.tile(sr.POS, (257, 1))) and not state[0].any()
    assert np.array_equal(state[1:], np.tile(sr.powers(8)[:, None], (1, 257)))


def test_identity_frame_reads_the_face_the_direction_points_at():
    """Face 2f + (d_f < 0) of the leading axis f, and a texel of the two other axes in cyclic order: a table that holds its own
    (F, iv, iu) gives them back."""
    R = 16
    F, iv, iu = np.meshgrid(np.arange(6), np.arange(R), np.arange(R), indexing="ij")
    g = np.stack([F, iv, iu], axis=-1).astype(np.float64)
    rays, state = sr.emit(0, 0, 4097, sr.POS, np.ones(3), None, R, g)
    d = rays[:, 3:]
    f = np.abs(d).argmax(axis=1)
    idx = np.arange(len(d))
    assert np.array_equal(state[1], 2 * f + (d[idx, f] < 0))
    u = d[idx, (f + 1) % 3] / np.abs(d[idx, f])
    v = d[idx, (f + 2) % 3] / np.abs(d[idx, f])
    assert np.array_equal(state[3], np.minimum(np.floor((u + 1.0) * 8.0), R - 1))
    assert np.array_equal(state[2], np.minimum(np.floor((v + 1.0) * 8.0), R - 1))


def test_the_device_cases_are_not_vacuous():
    """Over the frames, resolutions, seeds and first rays of tests/test_gpu_source.py (at its largest n): every cube face is read, a
    texel coordinate reaches R and is clamped, every class of tie between the leading axes occurs, and so does the NaN path."""
    faces, ties, clamped, nan = set(), set(), False, False
    per_frame = {}
    for name in sr.FRAMES:
        for R in sr.RES[1:]:
            for seed in sr.SEEDS:
                for first in sr.FIRST:
                    p = {}
                    sr.reference(seed, first, sr.SIZES[-1], 1, R, name, p)
                    faces |= p["faces"]
                    ties |= p["ties"]
                    clamped |= p["clamped"]
                    nan |= p["nan"]
                    per_frame.setdefault(name, []).append(p)
    assert faces == set(range(6))
    assert clamped and nan
    assert ties == {"all", "a0=a1", "a0=a2", "a1=a2"}
    assert all(p["faces"] == set(range(6)) for p in per_frame["identity"] + per_frame["rotation"] + per_frame["scaled_permutation"])
    assert all("all" in p["ties"] and p["clamped"] for p in per_frame["equal_rows"])
    assert all(p["nan"] and p["faces"] == {0} for p in per_frame["zero"])
