"""The point source on the MI355X (include/hare_hip.h, "receivers", "Source"): hare_emit_source's rays and starting state equal, byte
for byte, the numpy restatement tests/source_ref.py -- every size around the wave and the workgroup, first rays beyond 2^32, one to eight
bands, no table and three resolutions, seeds with every bit set and the sign bit alone, frames that are a rotation, a scaled
permutation, tied, and zero; nothing is written behind the rays or the state.  hare_receive_source is hare_receive_batch fed those rays
and that state, under the three partitions and in every mode of the loop; its scattering follows the global ray index; a burst split into
chunks sums to the one call; the sharded call is the one-device call; hare_emit_device allocates, frees and waits for nothing.
Status: written and checked against the reference on the CPU only (the kernel's source compiled for the host matches tests/source_ref.py
over the same axes); no MI355X could be had, so this file has not yet run on a device ("Source")."""
import numpy as np
import pytest

import hare_amd as H
from oracle import pyoracle as po
from tests import source_ref as sr
from tests.receive_ref import receive_loop
from tests.test_gpu_receivers import alpha_table, receivers, source
from tests.test_gpu_scattering import sigma_table

pytestmark = pytest.mark.gpu

N, CASTS = 4097, 4
N_BINS, BIN_LEN, FRAC = 400, 0.05, 40
GUARD = 64                                   # doubles behind the rays and behind the state
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def reference_directions():
    """The directions of the largest n for every (seed, first ray); a smaller n is their prefix (the chunk identity,
    tests/test_source_api.py)."""
    return {(seed, first): sr.directions(seed, first, sr.SIZES[-1])[0] for seed in sr.SEEDS for first in sr.FIRST}


@pytest.mark.parametrize("R", sr.RES)
@pytest.mark.parametrize("B", sr.BANDS)
def test_emit_device_matches_the_reference(torch, reference_directions, B, R):
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    power, table = sr.powers(B), sr.table(R, B) if R else None
    nmax = sr.SIZES[-1]
    d_rays = torch.empty(nmax * 6 + GUARD, dtype=torch.float64, device="cuda")
    d_state = torch.empty(nmax * (1 + B) + GUARD, dtype=torch.float64, device="cuda")
    for name, frame in sr.FRAMES.items():
        g.set_source(sr.POS, power=power, frame=frame, gain=table)
        assert (g.get_option("source_bands"), g.get_option("source_res")) == (B, R)
        for seed in sr.SEEDS:
            g.set_option("source_seed", seed)
            for first in sr.FIRST:
                d = reference_directions[seed, first]
                if R:
                    F, iv, iu, _ = sr.lookup(d, frame, R)
                    E = (power[None, :] * table[F, iv, iu, :]).T
                else:
                    E = np.tile((power * 1.0)[:, None], (1, nmax))
                for n in sr.SIZES:
                    d_rays.fill_(SENTINEL)
                    d_state.fill_(SENTINEL)
                    g.emit_device(n, d_rays.data_ptr(), d_state.data_ptr(), first_ray=first)
                    rays, state = d_rays.cpu().numpy(), d_state.cpu().numpy()
                    tag = (name, seed, first, n)
                    want = np.concatenate([np.tile(sr.POS, (n, 1)), d[:n]], axis=1)
                    assert rays[:n * 6].tobytes() == want.tobytes(), (tag, np.argwhere(rays[:n * 6].reshape(n, 6) != want)[:5])
                    assert np.all(rays[n * 6:] == SENTINEL), tag                     # nothing behind ray n
                    want_s = np.concatenate([np.zeros((1, n)), E[:, :n]], axis=0)
                    got_s = state[:n * (1 + B)].reshape(1 + B, n)                    # plane p ends where plane p + 1 begins: each is compared whole
                    assert got_s.tobytes() == want_s.tobytes(), (tag, np.argwhere(got_s != want_s)[:5])
                    assert np.all(state[n * (1 + B):] == SENTINEL), tag              # nothing behind the last plane
    # the whole path once more through the reference's own entry point
    rays, state = sr.reference(sr.SEEDS[1], sr.FIRST[1], 257, B, R, "rotation")
    g.set_source(sr.POS, power=power, frame=sr.FRAMES["rotation"], gain=table).set_option("source_seed", sr.SEEDS[1])
    g.emit_device(257, d_rays.data_ptr(), d_state.data_ptr(), first_ray=sr.FIRST[1])
    assert d_rays.cpu().numpy()[:257 * 6].tobytes() == rays.tobytes()
    assert d_state.cpu().numpy()[:257 * (1 + B)].tobytes() == state.tobytes()


# ---- hare_receive_source
B3, R3 = 3, 2


def partitions(T, To):
    return {"voxel": (lambda: H.Voxel_Grid([T], 8), lambda: po.VoxelGrid([To], domain=8)),
            "octree": (lambda: H.Octree([T], 4, 8), lambda: po.Octree([To], 4, 8)),
            "kdtree": (lambda: H.KDTree([T], 8, 6), lambda: po.KDTree([To], 8, 6))}


def shoebox_with_source(kind="voxel", seed=77, scatter=True):
    """The shoebox with five receivers, three bands of absorption (and scattering), and a directional source where
    hare_amd.scenes.burst_rays has its own."""
    m = H.scenes.shoebox()
    T, To = H.Topology(m.verts, m.nverts), po.Topology(m.verts, m.nverts)
    make, make_oracle = partitions(T, To)[kind]
    g = make()
    c, r = receivers(m.size)
    g.set_receivers(c, r).set_absorption(alpha_table(T.Polygon_Count, B3))
    if scatter:
        g.set_scattering(sigma_table(T.Polygon_Count, B3)).set_option("scatter_seed", 5)
    g.set_source(source(m.size), power=sr.powers(B3), frame=sr.FRAMES["rotation"], gain=sr.table(R3, B3)).set_option("source_seed", seed)
    return g, m, T, To, make_oracle, c, r


def emitted(m, seed, first, n):
    return sr.emit(seed, first, n, source(m.size), sr.powers(B3), sr.FRAMES["rotation"], R3, sr.table(R3, B3))


def same(a, b, what):
    for k, (x, y) in enumerate(zip(a[:4], b[:4])):                  # histogram, its float form, detections, final state
        assert x.tobytes() == y.tobytes(), (what, k, np.argwhere(x != y)[:5])
    assert a[4] == b[4], (what, a[4], b[4])                         # counters


@pytest.mark.parametrize("kind", ["voxel", "octree", "kdtree"])
def test_receive_source_is_receive_batch_fed_the_reference_rays(kind):
    g, m, T, To, _, c, r = shoebox_with_source(kind, scatter=False)
    rays, state = emitted(m, 77, 0, N)
    plain = g.Receive_source(N, CASTS, N_BINS, BIN_LEN, frac_bits=FRAC)
    same(plain, g.Receive_batch(rays, CASTS, N_BINS, BIN_LEN, energy=state, frac_bits=FRAC), (kind, "specular"))
    assert plain[2][:, 0].sum() > 0 and plain[3].tobytes() != state.tobytes()
    g.set_scattering(sigma_table(T.Polygon_Count, B3)).set_option("scatter_seed", 5)
    limited = None
    for what, kw, nb in (("scattering", {}, N_BINS), ("rain", dict(rain=True), N_BINS), ("directional", dict(directional=True), N_BINS),
                         ("rain, directional", dict(rain=True, directional=True), N_BINS), ("time limit", dict(time_limit=True), 60),
                         ("no time limit", {}, 60)):
        got = g.Receive_source(N, CASTS, nb, BIN_LEN, frac_bits=FRAC, **kw)
        same(got, g.Receive_batch(rays, CASTS, nb, BIN_LEN, energy=state, frac_bits=FRAC, **kw), (kind, what))
        assert got[2][:, 0].sum() > 0, (kind, what)
        if what == "scattering":
            assert got[0].tobytes() != plain[0].tobytes()
        if what == "time limit":
            limited = got
        if what == "no time limit":
            assert limited[4]["rays"] < got[4]["rays"] and np.array_equal(limited[0], got[0])      # the rule retired rays


def test_scattering_draws_follow_the_global_ray_index():
    first = 2 ** 32 - 100
    g, m, T, To, make_oracle, c, r = shoebox_with_source("voxel", seed=-3)
    rays, state = emitted(m, -3, first, N)
    want_h, want_d, want_s, _ = receive_loop(po, To, make_oracle(), rays, CASTS, c, r, N_BINS, BIN_LEN, FRAC, alpha=alpha_table(T.Polygon_Count, B3),
                                            sigma=sigma_table(T.Polygon_Count, B3), seed=5, state_in=state, g0=first)
    hist, _, det, state_out, _ = g.Receive_source(N, CASTS, N_BINS, BIN_LEN, first_ray=first, frac_bits=FRAC)
    assert want_d[:, 0].sum() > 0
    assert np.array_equal(det, want_d) and np.array_equal(hist, want_h), np.argwhere(hist != want_h)[:5]
    assert state_out.tobytes() == want_s.tobytes()
    # the same rays counted from 0 scatter otherwise
    other = g.Receive_batch(rays, CASTS, N_BINS, BIN_LEN, energy=state, frac_bits=FRAC)
    assert other[3].tobytes() != state_out.tobytes()


@pytest.mark.parametrize("first", [0, 2 ** 40])
def test_chunks_sum_to_the_one_call(first):
    g, m, T, To, _, c, r = shoebox_with_source("voxel")
    quiet = g.Receive_source(N, 8, N_BINS, BIN_LEN, first_ray=first, frac_bits=FRAC)
    g.set_option("receive_floor_bits", 2).set_option("receive_roulette", 1)
    one = g.Receive_source(N, 8, N_BINS, BIN_LEN, first_ray=first, frac_bits=FRAC)
    assert one[4]["rays"] < quiet[4]["rays"] and one[3].tobytes() != quiet[3].tobytes()        # the roulette played
    k = 1500
    a = g.Receive_source(k, 8, N_BINS, BIN_LEN, first_ray=first, frac_bits=FRAC)
    b = g.Receive_source(N - k, 8, N_BINS, BIN_LEN, first_ray=first + k, frac_bits=FRAC)
    assert np.array_equal(a[0] + b[0], one[0]) and np.array_equal(a[2] + b[2], one[2])
    assert np.concatenate([a[3], b[3]], axis=1).tobytes() == one[3].tobytes()
    assert {f: a[4][f] + b[4][f] for f in ("rays", "hits")} == {f: one[4][f] for f in ("rays", "hits")}


def test_sharded_call_is_the_one_scene_call():
    made = [shoebox_with_source("voxel") for _ in range(2)]
    parts = [x[0] for x in made]
    first = 2 ** 32 - 100
    one = parts[0].Receive_source(N, CASTS, N_BINS, BIN_LEN, first_ray=first, frac_bits=FRAC)
    two = H.Voxel_Grid.Receive_source_sharded(parts, N, CASTS, N_BINS, BIN_LEN, first_ray=first, frac_bits=FRAC)
    same(one, two, "sharded")
    assert one[2][:, 0].sum() > 0
    parts[1].set_option("source_seed", 78)
    with pytest.raises(H.HareError) as ei:
        H.Voxel_Grid.Receive_source_sharded(parts, N, CASTS, N_BINS, BIN_LEN, frac_bits=FRAC)
    assert ei.value.code == H.capi.HARE_E_INVALID


def test_emit_device_allocates_frees_and_waits_for_nothing(torch):
    g, m, *_ = shoebox_with_source("voxel")
    n = 4159
    d_rays = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    d_state = torch.empty((1 + B3, n), dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        names = ("hip_malloc_calls", "hip_free_calls", "hip_sync_calls")
        before = [g.get_option(k) for k in names]
        g.emit_device(n, d_rays.data_ptr(), d_state.data_ptr(), first_ray=9, stream=s.cuda_stream)
        assert [g.get_option(k) for k in names] == before
        s.synchronize()
    rays, state = emitted(m, 77, 9, n)
    assert d_rays.cpu().numpy().tobytes() == rays.tobytes() and d_state.cpu().numpy().tobytes() == state.tobytes()
