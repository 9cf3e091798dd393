"""Receiver maps on the MI355X (include/hare_hip.h, "receivers", "Receiver maps"): every case of tests.receive_map_ref.map_cases() --
K = 1 .. 65 536, batch sizes about a wave, a workgroup and 4096, B = 1, 3, 8, one to four casts, the four _map kernels, the three
partitions, shoebox, partition room and an open soup, the six map shapes, states with NaN and infinities beside directions scaled by
2^-600 (NaN and infinite RAYS reach the device in tests/test_gpu_receive_map_edges.py and tests/test_gpu_receive_map_sweep.py, with the
visit rule's other edges; no cast is shot with them here), the time limit and the floor with roulette -- through Receive_batch and, for a subset, receive_device on the caller's buffers
and the sharded call over two scenes.  Histogram, detections and final state (for the device call also the rays and the last events)
equal the numpy restatement (tests/receive_ref.py with tests/receive_map_ref.py's visit rule) byte for byte; of a NaN only that it is
one is compared.  Nothing is skipped or redrawn.  tests/test_receive_map_api.py proves with the restatement alone that the cases are not vacuous.  Further: the identity (the
same K <= 256 receivers through both setters give the same bytes, omni and directional, with and without scattering); chunks of
hare_receive_source sum to the one call; the receive call with a map allocates and frees nothing."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests.receive_cases import mesh_of, reference
from tests.receive_harness import check_case, library_partitions, run_batch, same_bits
from tests.receive_map_ref import identity_cases, map_case, map_cases

pytestmark = pytest.mark.gpu

CASES = map_cases()
IDENTITY = identity_cases()


@pytest.mark.parametrize("mc", CASES, ids=[c.name for c in CASES])
def test_case_equals_the_reference(mc):
    seen = {}
    bad = check_case(mc, reference(mc, keep=True), seen=seen)        # Receive_batch; receive_device and two scenes where the case asks
    assert seen["parts"][0].get_option("receiver_map") == 1
    assert bad is None, (mc.describe(), bad)
    if mc.device:
        assert seen["calls"] == [0, 0, 0], seen["calls"]            # stream-ordered: no allocation, no free, no wait, whatever the casts


@pytest.mark.parametrize("mc", IDENTITY, ids=[c.name for c in IDENTITY])
def test_the_same_receivers_through_both_setters_give_the_same_bytes(mc):
    h1, d1, s1 = run_batch(mc, library_partitions(mc))
    h0, d0, s0 = run_batch(mc, library_partitions(mc, linear=True))
    assert d0[:, 0].sum() > 0 and h0.any()
    for got, ref in ((h1, h0), (d1, d0), (s1, s0)):
        assert same_bits(got, ref) is None, (mc.describe(), same_bits(got, ref))
    # ... and on one scene, switching back and forth
    p = library_partitions(mc)[0]
    p.set_receivers(mc.centers, mc.radii)
    assert p.get_option("receiver_map") == 0
    h2, d2, s2 = run_batch(mc, [p])
    p.set_receiver_map(mc.centers, mc.radii, mc.map_cell)
    h3, d3, s3 = run_batch(mc, [p])
    for got in ((h2, d2, s2), (h3, d3, s3)):
        assert all(same_bits(a, b) is None for a, b in zip(got, (h0, d0, s0)))


def test_chunks_of_receive_source_sum_to_the_one_call():
    case = map_case("source", "plane", 1000, 4097, B=3, bounces=3, mode="scatter")
    p = library_partitions(case)[0]
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
        p.Receive_batch(mc.rays, 2, mc.n_bins, mc.bin_len, rain=True)
    assert ei.value.code == capi.HARE_E_INVALID
