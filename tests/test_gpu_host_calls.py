"""The host-buffer calls' split of a batch on the device: the four _sharded calls over three scenes against the single-scene call on a fourth,
and hare_shoot_batch / hare_occluded_batch under "batch_chunks" = 1, 3 and 16 against each other -- byte for byte, counters included.
n = 1 and 2 leave shards empty, 5 and 37 give uneven ones (37 in 16 chunks: chunks of 2 and 3), 4097 is one past the bounce loop's block list."""
import ctypes as C

import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 5, 37, 4097)
BOUNCES = 3


@pytest.fixture(scope="module")
def box():
    return H.scenes.shoebox()


@pytest.fixture(scope="module")
def scenes(box):
    """three scenes on the one device and the reference scene, all with the same receiver"""
    gs = [H.Voxel_Grid([H.Topology(box.verts, box.nverts)], 8) for _ in range(4)]
    for g in gs:
        g.set_receivers([[5.0, 3.5, 2.0]], [0.5])
    yield gs[:3], gs[3]
    for g in gs:
        g.close()


@pytest.fixture(scope="module")
def rays(box):
    return H.scenes.random_rays(max(SIZES), box.size)


def ctr_bytes(c):
    return bytes(c)


def occluded(gs, rays, tmax, events):
    """hare_occluded_batch (one scene) or hare_occluded_batch_sharded: (flags, events, counters bytes)"""
    n = len(rays)
    occ, out, ctr = np.full(n, -7, np.int32), (np.zeros(n, capi.XEVENT_DTYPE) if events else None), capi.Counters()
    if len(gs) == 1:
        rc = capi.lib.hare_occluded_batch(gs[0]._h, gs[0]._kind, 0, n, capi.ptr(rays), None, None, capi.ptr(tmax), 0, capi.ptr(occ), capi.ptr(out), C.addressof(ctr))
    else:
        h = (C.c_void_p * len(gs))(*[g._h for g in gs])
        rc = capi.lib.hare_occluded_batch_sharded(h, len(gs), gs[0]._kind, 0, n, capi.ptr(rays), None, None, capi.ptr(tmax), 0, capi.ptr(occ), capi.ptr(out),
                                                  C.addressof(ctr))
    capi.check(rc)
    return occ, out, ctr_bytes(ctr)


def shoot_raw(gs, rays, flags=0):
    """hare_shoot_batch / _sharded with the whole counter block: (events or slim records, counters bytes)"""
    n = len(rays)
    out, ctr = np.zeros(n, gs[0]._slim_dtype() if flags & capi.SHOOT_SLIM_EVENTS else capi.XEVENT_DTYPE), capi.Counters()
    if len(gs) == 1:
        rc = capi.lib.hare_shoot_batch(gs[0]._h, gs[0]._kind, 0, n, capi.ptr(rays), None, None, flags, capi.ptr(out), C.addressof(ctr))
    else:
        h = (C.c_void_p * len(gs))(*[g._h for g in gs])
        rc = capi.lib.hare_shoot_batch_sharded(h, len(gs), gs[0]._kind, 0, n, capi.ptr(rays), None, None, flags, capi.ptr(out), C.addressof(ctr))
    capi.check(rc)
    return out, ctr_bytes(ctr)


@pytest.mark.parametrize("n", SIZES)
def test_shoot_sharded_is_the_single_scene_call(scenes, rays, n):
    three, ref = scenes
    r = np.ascontiguousarray(rays[:n])
    for flags in (0, capi.SHOOT_COUNT_WORK, capi.SHOOT_SLIM_EVENTS):
        want, want_ctr = shoot_raw([ref], r, flags)
        got, got_ctr = shoot_raw(three, r, flags)
        assert got.tobytes() == want.tobytes() and got_ctr == want_ctr, flags
    assert want_ctr[:8] == np.uint64(n).tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_occluded_sharded_is_the_single_scene_call(scenes, rays, n):
    three, ref = scenes
    r = np.ascontiguousarray(rays[:n])
    tmax = np.linspace(0.5, 6.0, n)
    for events in (False, True):
        want = occluded([ref], r, tmax, events)
        got = occluded(three, r, tmax, events)
        assert got[0].tobytes() == want[0].tobytes() and got[2] == want[2]
        assert np.isin(got[0], (0, 1)).all()
        if events:
            assert got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_bounce_sharded_is_the_single_scene_call(scenes, rays, n):
    three, ref = scenes
    r = np.ascontiguousarray(rays[:n])
    for every in (False, True):
        want, want_ctr, want_pc = ref.Bounce_batch(r, BOUNCES, all_casts=every, per_cast=True)
        ev = np.zeros((BOUNCES, n) if every else n, capi.XEVENT_DTYPE)
        h, ctr, pcs = (C.c_void_p * 3)(*[g._h for g in three]), capi.Counters(), (capi.Counters * BOUNCES)()
        capi.check(capi.lib.hare_bounce_batch_sharded(h, 3, ref._kind, 0, n, capi.ptr(r), None, None, BOUNCES, 0, capi.ptr(ev) if every else None,
                                                      None if every else capi.ptr(ev), C.addressof(ctr), C.addressof(pcs)))
        assert ev.tobytes() == want.tobytes()
        assert ctr.as_dict() == want_ctr and [pcs[b].as_dict() for b in range(BOUNCES)] == want_pc
        assert want_pc[0]["rays"] == n


@pytest.mark.parametrize("n", SIZES)
def test_receive_sharded_is_the_single_scene_call(scenes, rays, n):
    three, ref = scenes
    r = np.ascontiguousarray(rays[:n])
    want = ref.Receive_batch(r, BOUNCES, 16, 2.0)
    got = H.Spatial_Partition.Receive_batch_sharded(three, r, BOUNCES, 16, 2.0)
    for w, g in zip(want[:4], got[:4]):
        assert g.tobytes() == w.tobytes()
    assert got[4] == want[4] and want[4]["rays"] > 0


@pytest.mark.parametrize("n", (37, 4097))
def test_the_chunk_count_changes_nothing(scenes, rays, n):
    _, g = scenes
    r = np.ascontiguousarray(rays[:n])
    tmax = np.linspace(0.5, 6.0, n)
    seen = []
    try:
        for chunks in (1, 3, 16):
            g.set_option("batch_chunks", chunks)
            ev, ctr = shoot_raw([g], r, capi.SHOOT_COUNT_WORK)
            slim, slim_ctr = shoot_raw([g], r, capi.SHOOT_SLIM_EVENTS)
            occ = occluded([g], r, tmax, False)
            occ_ev = occluded([g], r, tmax, True)
            seen.append((ev.tobytes(), ctr, g.expand_events(r, slim).tobytes(), slim.tobytes(), slim_ctr, occ[0].tobytes(), occ[2], occ_ev[0].tobytes(),
                         occ_ev[1].tobytes(), occ_ev[2]))
    finally:
        g.set_option("batch_chunks", 0)
    assert seen[0] == seen[1] == seen[2]
    assert seen[0][2] == shoot_raw([g], r)[0].tobytes()          # the expanded slim records are the X_Events
    assert np.frombuffer(seen[0][0], capi.XEVENT_DTYPE)["hit"].any()
