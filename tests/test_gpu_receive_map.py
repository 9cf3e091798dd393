"""Receiver maps on the MI355X (include/hare_hip.h, "receivers", "Receiver maps"): every case of tests.receive_map_ref.map_cases() --
K = 1 .. 65 536, batch sizes about a wave, a workgroup and 4096, B = 1, 3, 8, one to four casts, the four _map kernels, the three
partitions, shoebox, partition room and an open soup, the six map shapes, states with NaN and infinities beside directions scaled by
2^-600 (NaN and infinite RAYS meet the visit rule in tests/test_receive_map_api.py, on the restatement: no cast is shot with them here), the time limit and the floor with roulette -- through Receive_batch and, for a subset, receive_device on the caller's buffers
and the sharded call over two scenes.  Histogram, detections and final state (for the device call also the rays and the last events)
equal the numpy restatement (tests/receive_map_ref.py) byte for byte; of a NaN only that it is one is compared.  Nothing is skipped or
redrawn.  tests/test_receive_map_api.py proves with the restatement alone that the cases are not vacuous.  Further: the identity (the
same K <= 256 receivers through both setters give the same bytes, omni and directional, with and without scattering); chunks of
hare_receive_source sum to the one call; the receive call with a map allocates and frees nothing."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests.receive_cases import mesh_of
from tests.receive_cut_ref import same_bits
from tests.receive_map_ref import map_case, map_cases, reference

pytestmark = pytest.mark.gpu

CASES = map_cases()


def library_partitions(mc, count=1, linear=False):
    case = mc.case
    verts, nverts, _ = mesh_of(case.scene)
    T = H.Topology(verts, nverts)
    kind, *par = case.partition
    parts = []
    for _ in range(count):
        p = H.Voxel_Grid([T], par[0]) if kind == "voxel" else (H.Octree if kind == "octree" else H.KDTree)([T], *par)
        if linear:
            p.set_receivers(case.centers, case.radii)
        else:
            p.set_receiver_map(case.centers, case.radii, mc.cell)
        if case.alpha is not None:
            p.set_absorption(case.alpha)
        if case.sigma is not None:
            p.set_scattering(case.sigma)
        p.set_option("scatter_seed", case.seed).set_option("receive_floor_bits", mc.floor_bits).set_option("receive_roulette", int(mc.roulette))
        parts.append(p)
    return parts


def run_batch(mc, parts):
    case = mc.case
    kw = dict(energy=case.state_in, frac_bits=case.frac_bits, directional=case.directional, time_limit=mc.time_limit)
    if len(parts) == 1:
        hist, _, det, state, _ = parts[0].Receive_batch(case.rays, case.bounces, case.n_bins, case.bin_len, **kw)
    else:
        hist, _, det, state, _ = type(parts[0]).Receive_batch_sharded(parts, case.rays, case.bounces, case.n_bins, case.bin_len, **kw)
    return hist, det, state


def run_device(mc, part):
    """receive_device on the caller's buffers, accumulators zeroed: dict of hist, det, state, rays, events, and the HIP call counters'
    change over the call."""
    import torch
    case = mc.case
    n, K, B = case.n, case.K, case.B
    state = case.state_in if case.state_in is not None else np.concatenate([np.zeros((1, n)), np.ones((B, n))])
    d_rays = torch.from_numpy(np.ascontiguousarray(case.rays)).to("cuda")
    d_state = torch.from_numpy(np.ascontiguousarray(state)).to("cuda")
    d_work = torch.zeros(H.Voxel_Grid.receive_work_bytes(n), dtype=torch.uint8, device="cuda")
    d_last = torch.zeros(n * 56, dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros(case.words, dtype=torch.int64, device="cuda")
    d_det = torch.zeros(2 * K, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    before = [part.get_option(o) for o in ("hip_malloc_calls", "hip_free_calls", "hip_sync_calls")]
    part.receive_device(n, d_rays.data_ptr(), case.bounces, case.n_bins, case.bin_len, case.frac_bits, d_state.data_ptr(), d_work.data_ptr(),
                        d_last.data_ptr(), d_hist.data_ptr(), d_det.data_ptr(), directional=case.directional, time_limit=mc.time_limit)
    after = [part.get_option(o) for o in ("hip_malloc_calls", "hip_free_calls", "hip_sync_calls")]
    torch.cuda.synchronize()
    shape = (K, case.n_bins, B, 4) if case.directional else (K, case.n_bins, B)
    return dict(hist=d_hist.cpu().numpy().view(np.uint64).reshape(shape), det=d_det.cpu().numpy().view(np.uint64).reshape(K, 2),
                state=d_state.cpu().numpy(), rays=d_rays.cpu().numpy(),
                events=np.frombuffer(d_last.cpu().numpy().tobytes(), dtype=capi.XEVENT_DTYPE),
                calls=[a - b for a, b in zip(after, before)])


def mismatch(want, hist, det, state, rays=None, events=None):
    for what, got, ref in (("detections", det, want["det"]), ("histogram", hist, want["hist"]), ("state", state, want["state"])):
        bad = same_bits(got, ref)
        if bad:
            return f"{what}: {bad}"
    if rays is not None:
        bad = same_bits(rays, want["rays"])
        if bad:
            return f"rays: {bad}"
    if events is not None:
        for f in events.dtype.names:
            bad = same_bits(events[f], want["events"][f])
            if bad:
                return f"last X_Event.{f}: {bad}"
    return None


@pytest.mark.parametrize("mc", CASES, ids=[c.name for c in CASES])
def test_case_equals_the_reference(mc):
    want = reference(mc)
    parts = library_partitions(mc)
    assert parts[0].get_option("receiver_map") == 1
    hist, det, state = run_batch(mc, parts)
    bad = mismatch(want, hist, det, state)
    assert bad is None, (mc.describe(), "Receive_batch", bad)
    if mc.call == "device":
        got = run_device(mc, parts[0])
        bad = mismatch(want, got["hist"], got["det"], got["state"], got["rays"], got["events"])
        assert bad is None, (mc.describe(), "receive_device", bad)
        assert got["calls"] == [0, 0, 0], got["calls"]          # stream-ordered: no allocation, no free, no wait, whatever the casts
    if mc.call == "sharded":
        hist, det, state = run_batch(mc, library_partitions(mc, count=2))
        bad = mismatch(want, hist, det, state)
        assert bad is None, (mc.describe(), "Receive_batch_sharded", bad)


IDENTITY = [map_case("identity-omni", "plane", 256, 4097, B=3, bounces=4),
            map_case("identity-dir", "cloud", 200, 4097, B=3, bounces=3, directional=True, partition="octree"),
            map_case("identity-scatter", "coincident", 256, 4097, B=8, bounces=3, mode="scatter", scene=("room",)),
            map_case("identity-scatter-dir", "cell", 255, 257, B=1, bounces=4, mode="scatter", directional=True, partition="kdtree")]


@pytest.mark.parametrize("mc", IDENTITY, ids=[c.name for c in IDENTITY])
def test_the_same_receivers_through_both_setters_give_the_same_bytes(mc):
    h1, d1, s1 = run_batch(mc, library_partitions(mc))
    h0, d0, s0 = run_batch(mc, library_partitions(mc, linear=True))
    assert d0[:, 0].sum() > 0 and h0.any()
    for got, ref in ((h1, h0), (d1, d0), (s1, s0)):
        assert same_bits(got, ref) is None, (mc.describe(), same_bits(got, ref))
    # ... and on one scene, switching back and forth
    p = library_partitions(mc)[0]
    p.set_receivers(mc.case.centers, mc.case.radii)
    assert p.get_option("receiver_map") == 0
    h2, d2, s2 = run_batch(mc, [p])
    p.set_receiver_map(mc.case.centers, mc.case.radii, mc.cell)
    h3, d3, s3 = run_batch(mc, [p])
    for got in ((h2, d2, s2), (h3, d3, s3)):
        assert all(same_bits(a, b) is None for a, b in zip(got, (h0, d0, s0)))


def test_chunks_of_receive_source_sum_to_the_one_call():
    mc = map_case("source", "plane", 1000, 4097, B=3, bounces=3, mode="scatter")
    case = mc.case
    p = library_partitions(mc)[0]
    p.set_source(np.array([0.31, 0.42, 0.37]) * np.asarray(mesh_of(case.scene)[2]), power=[1.0, 0.5, 0.25])
    lib, n = capi.lib, case.n
    K, B = case.K, case.B

    def call(first, count):
        hist, det = np.zeros((K, case.n_bins, B), np.uint64), np.zeros((K, 2), np.uint64)
        capi.check(lib.hare_receive_source(p._h, p._kind, 0, count, first, case.bounces, 0, case.n_bins, case.bin_len, case.frac_bits, None,
                                           capi.ptr(hist), capi.ptr(det), None))
        return hist, det
    h, d = call(0, n)
    assert d[:, 0].sum() > 0 and (d[:, 0] > 0).sum() > 50          # spread over the map
    parts = [call(0, 1000), call(1000, 2049), call(3049, n - 3049)]
    assert same_bits(sum(x[0] for x in parts), h) is None and same_bits(sum(x[1] for x in parts), d) is None


def test_rain_with_a_map_is_refused_on_the_device_too():
    mc = map_case("rain", "plane", 256, 63, B=3, bounces=2, mode="scatter")
    p = library_partitions(mc)[0]
    with pytest.raises(H.HareError) as ei:
        p.Receive_batch(mc.case.rays, 2, mc.case.n_bins, mc.case.bin_len, rain=True)
    assert ei.value.code == capi.HARE_E_INVALID
