"""The direct sound on the CPU (include/hare_hip.h, "receivers", "Direct sound"): that the device cases of tests/test_gpu_direct.py hold
every class of the definition (asserted with tests/direct_ref.py alone, so that the device tests cannot pass vacuously); that f * W is the
number of a burst's rays that pass through the sphere -- the one thing a byte comparison cannot see, as reference and kernel share the
formula; and the refusals and the check order of hare_direct_device and of HARE_RECEIVE_DIRECT on every receive call."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests import direct_ref as dr
from tests import receive_ref as rr
from tests import source_ref as sr

E_INVALID, E_NODEVICE, E_STATE = capi.HARE_E_INVALID, capi.HARE_E_NODEVICE, capi.HARE_E_STATE


def code(call):
    try:
        call()
    except H.HareError as e:
        return e.code
    return capi.HARE_OK


# ---- (a) coverage
@pytest.fixture(scope="module")
def references():
    return {c.name: (c, dr.reference(c)) for c in dr.cases()}


def test_cases_span_the_axes():
    cs = dr.cases()
    assert {c.partition[0] for c in cs} == {"voxel", "octree", "kdtree"}
    assert {c.K for c in cs if not c.map} == {1, 3, 64, 255, 256} and {c.K for c in cs if c.map} == {257, 4096}
    assert {c.B for c in cs} == {1, 3, 8} and {c.R for c in cs} == {0, 1, 4} and {c.frac_bits for c in cs} == {0, 40, 62}
    assert {c.n_bins for c in cs} >= {1, 4096} and {c.directional for c in cs} == {False, True}
    assert {c.n_weight for c in cs} == {1, 4097, 2 ** 40}
    assert all(c.K * c.n_bins * c.B * (4 if c.directional else 1) <= 1 << 27 for c in cs)


def test_cases_hold_every_class_of_the_definition(references):
    some = lambda f: [n for n, (c, r) in references.items() if f(c, r)]
    seen = lambda key: some(lambda c, r: bool(r["seen"][key].any()))
    assert seen("occluded") and seen("binned") and seen("edge")
    assert some(lambda c, r: bool((~r["seen"]["eligible"]).any()))                                   # the source inside a sphere
    assert some(lambda c, r: bool((r["seen"]["eligible"] & ~r["seen"]["occluded"] & ~r["seen"]["binned"]).any()))      # unbinned
    assert some(lambda c, r: c.frac_bits == 62 and r["tallies"].get("saturated", 0) > 0)
    assert some(lambda c, r: r["tallies"].get("round_to_zero", 0) > 0)
    assert some(lambda c, r: r["tallies"].get("zeroed_zero", 0) > 0 and c.B >= 3)                     # powers(B)[2] = 0
    faces = set()
    for c, r in references.values():
        faces |= r["seen"]["faces"]
    assert faces == set(range(6))
    # every multi-receiver case has both a deposit and an occluded receiver; detections count the visible receivers, each once
    for name, (c, r) in references.items():
        s = r["seen"]
        vis = s["eligible"] & ~s["occluded"]
        assert (r["det"].sum(axis=1) == vis.astype(np.uint64)).all(), name
        assert (r["det"][:, 0] == s["binned"].astype(np.uint64)).all(), name
        if c.K >= 64:
            assert s["occluded"].any() and s["binned"].any(), name
        if c.directional and c.frac_bits < 62:                      # |X|, |Y|, |Z| <= W + 1/2 per add: one add per word here
            w = r["hist"][..., 0].astype(np.float64)
            assert (np.abs(H.Spatial_Partition.directional_signed(r["hist"]).astype(np.float64)) <= w[..., None] + 1).all(), name


def test_the_share_has_no_cancellation_and_the_right_limits():
    d2 = np.array([1.0, 4.0, 1e6, 1e30])
    f = dr.share(np.float64(0.25), d2)
    assert np.allclose(f, 0.25 / (4.0 * d2), rtol=0.1) and f[3] > 0 and f[3] == 0.0625 / 1e30          # far away: r^2 / 4 d^2, no loss
    assert dr.share(np.float64(1.0), np.nextafter(1.0, 2.0)) <= 0.5                                   # a sphere that touches the source: half


# ---- (b) the scale of f * W
SEEDS = (0, 11, 2024)
N_BURST = 65536


def test_the_deposit_is_the_expected_count_of_a_burst():
    """8 receivers in the shoebox, wholly inside it (a ray's closest approach to a center that lies in a sphere inside a convex room comes
    before its wall hit, so cast 0's t_end is immaterial), f between 0.005 and 0.07.  Cast 0's detections of a 65 536-ray burst per
    receiver against n f: within 4.5 sigma of the binomial for three fixed seeds (24 pairs; a factor wrong misses by tens of sigma)."""
    pos = np.array([4.0, 3.0, 2.0])
    radii = np.array([0.5, 0.5, 0.4, 0.4, 0.3, 0.45, 0.35, 0.3])
    dists = np.array([1.0, 1.5, 1.0, 1.5, 1.0, 2.5, 2.4, 2.0])
    u = np.random.default_rng(5).normal(size=(8, 3))
    u[:, 2] *= 0.3                                                     # flat: the room is 4 high
    u /= np.linalg.norm(u, axis=1)[:, None]
    centers = pos + u * dists[:, None]
    assert ((centers - radii[:, None] > 0) & (centers + radii[:, None] < np.array([10.0, 7.0, 4.0]))).all()
    v = centers - pos
    f = dr.share(radii * radii, (v * v).sum(axis=1))
    assert (f > 0.005).all() and (f < 0.07).all() and f.min() < 0.007 and f.max() > 0.06
    for seed in SEEDS:
        rays, state = sr.emit(seed, 0, N_BURST, pos, [1.0], None, 0, None)
        hist, det = np.zeros((8, 1, 1), np.uint64), np.zeros((8, 2), np.uint64)
        rr.receiver_step(rays[:, :3], rays[:, 3:], np.full(N_BURST, np.inf), state[0], state[1:], centers, radii, 1, 100.0, 0, hist, det)
        count = det.sum(axis=1).astype(np.float64)
        sigma = np.sqrt(N_BURST * f * (1 - f))
        print(seed, np.round((count - N_BURST * f) / sigma, 2))
        assert (np.abs(count - N_BURST * f) <= 4.5 * sigma).all(), (seed, count, N_BURST * f)


# ---- (c) refusals and check order
def grid():
    m = H.scenes.shoebox()
    return H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8), m


def test_direct_device_checks_in_order(gpu_available):
    g, m = grid()
    lib, h = capi.lib, g._h
    W, HI, D = 1 << 20, 2 << 20, 3 << 20                                # addresses are only compared before a device is found

    def call(n_weight=5, n_bins=8, bin_len=0.5, frac_bits=20, work=W, hist=HI, det=D, kind=capi.KIND_VOXEL, top=0, flags=0):
        return lib.hare_direct_device(h, kind, top, n_weight, flags, n_bins, bin_len, frac_bits, work, hist, det, None)
    for bad in (dict(n_weight=0), dict(n_weight=-1), dict(n_weight=2 ** 53 + 1), dict(n_bins=0), dict(bin_len=0.0), dict(bin_len=float("nan")),
                dict(frac_bits=-1), dict(frac_bits=63), dict(kind=7), dict(top=1), dict(n_bins=2 ** 27 + 1), dict(n_bins=2 ** 25 + 1, flags=256),
                dict(work=None), dict(hist=None), dict(det=None), dict(hist=W + 64), dict(det=W + 300), dict(det=HI + 8)):
        assert call(**bad) == E_INVALID, bad
    assert call(n_weight=2 ** 53, work=W, hist=W + 320, det=W + 320 + 64) == (E_STATE if gpu_available else E_NODEVICE)     # 64 K + 256, 8 words, then 2
    g.set_receivers([np.asarray(m.size) * 0.5] * 2, [0.5, 0.25])
    assert call(det=HI + 2 * 8 * 8 - 8) == E_INVALID and call(work=W, hist=W + 64 * 2 + 255) == E_INVALID                   # sizes follow K
    assert call() == (E_STATE if gpu_available else E_NODEVICE)
    if gpu_available:
        assert "no source" in capi.last_error()
    g.set_source(np.asarray(m.size) * 0.3, power=np.ones(3))
    assert call() == E_INVALID and "bands" in capi.last_error()         # before any device is looked for
    g.set_absorption(np.full((g.Model[0].Polygon_Count, 3), 0.1))
    if not gpu_available:
        assert call() == E_NODEVICE
    assert H.Voxel_Grid.direct_work_bytes(2) == 64 * 2 + 256


def test_the_flag_is_refused_on_the_batch_calls_and_checked_in_order_on_the_others(gpu_available):
    g, m = grid()
    g.set_receivers([np.asarray(m.size) * 0.5], [0.5])
    rays = H.scenes.random_rays(8, m.size)
    lib, h = capi.lib, g._h
    FLAG = capi.RECEIVE_DIRECT
    assert FLAG == 1024
    hist, det, ctr = np.zeros(10, np.uint64), np.zeros(2, np.uint64), capi.Counters()
    import ctypes as C
    batch = lambda flags: lib.hare_receive_batch(h, g._kind, 0, 8, capi.ptr(rays), None, None, 2, flags, 10, 0.1, 20, None, None, capi.ptr(hist),
                                                 capi.ptr(det), C.addressof(ctr))
    assert batch(FLAG) == E_INVALID and "HARE_RECEIVE_DIRECT" in capi.last_error()
    assert batch(FLAG | capi.RECEIVE_DIRECTIONAL) == E_INVALID
    handles = (C.c_void_p * 1)(h)
    assert lib.hare_receive_batch_sharded(handles, 1, g._kind, 0, 8, capi.ptr(rays), None, None, 2, FLAG, 10, 0.1, 20, None, None, capi.ptr(hist),
                                          capi.ptr(det), C.addressof(ctr)) == E_INVALID
    sums, win = np.zeros(4, np.uint64), np.array([0, 10], np.int32)
    assert lib.hare_receive_batch_reduced(h, g._kind, 0, 8, capi.ptr(rays), None, None, 2, FLAG, 10, 0.1, 20, None, None, None, 1, capi.ptr(win), 0,
                                          None, capi.ptr(sums), None, capi.ptr(det), C.addressof(ctr)) == E_INVALID
    if not gpu_available:
        assert batch(0) == E_NODEVICE                                                  # nothing else about the call has moved
    # the source calls: their own checks first, then the device, then the state (no source)
    assert code(lambda: g.Receive_source(16, 2, 10, 0.0, direct=True)) == E_INVALID
    assert code(lambda: g.Receive_source(16, 2, 10, 0.1, direct=True)) == (E_STATE if gpu_available else E_NODEVICE)
    assert code(lambda: g.Receive_source_reduced(16, 2, 10, 0.1, windows=[(0, 10)], direct=True)) == (E_STATE if gpu_available else E_NODEVICE)
    if gpu_available:
        assert "no source" in capi.last_error()
    dev = lambda: g.receive_device(8, 1 << 20, 2, 10, 0.1, 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20, direct=True)
    assert code(dev) == (E_STATE if gpu_available else E_NODEVICE)
    g.set_source(np.asarray(m.size) * 0.3, power=np.ones(3))
    assert code(lambda: g.Receive_source(16, 2, 10, 0.1, direct=True)) == E_INVALID and "bands" in capi.last_error()
    assert code(dev) == E_INVALID and "bands" in capi.last_error()
    g2, _ = grid()
    g2.set_receivers([np.asarray(m.size) * 0.5], [0.5]).set_source(np.asarray(m.size) * 0.3)
    g.set_source(np.asarray(m.size) * 0.3)
    both = lambda: H.Spatial_Partition.Receive_source_sharded([g, g2], 16, 2, 10, 0.1, direct=True)
    assert code(both) == (capi.HARE_OK if gpu_available else E_NODEVICE)
