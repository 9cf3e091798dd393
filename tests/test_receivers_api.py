"""Receivers (include/hare_hip.h, "receivers") without a GPU: the new exports are bound, every bad argument is HARE_E_INVALID before
anything runs, the setters work on a GPU-less scene and read back, a receive call without a device is HARE_E_NODEVICE, and the numpy
restatement the GPU tests compare against (tests/receive_ref.py) gives the hand-worked answers on the edge cases of the definition."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests.receive_ref import quantise, receiver_step

NEW = ("hare_scene_set_receivers", "hare_scene_set_absorption", "hare_receive_device", "hare_receive_batch", "hare_receive_batch_sharded")


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


def test_setters_validate_and_read_back_without_a_gpu():
    g, T = grid()
    assert g.get_option("receivers") == 0 and g.get_option("bands") == 1
    ok_c, ok_r = np.zeros((2, 3)), np.ones(2)
    for centers, radii in [(np.zeros((0, 3)), np.zeros(0)), (np.zeros((257, 3)), np.ones(257)),
                           ([[np.nan, 0, 0]], [1.0]), ([[0, np.inf, 0]], [1.0]), ([[0, 0, 0]], [0.0]), ([[0, 0, 0]], [-1.0]),
                           ([[0, 0, 0]], [np.inf]), ([[0, 0, 0]], [np.nan])]:
        with pytest.raises(H.HareError) as ei:
            g.set_receivers(centers, radii)
        assert ei.value.code == capi.HARE_E_INVALID
    assert g.get_option("receivers") == 0            # a refused call changes nothing
    g.set_receivers(ok_c, ok_r)
    assert g.get_option("receivers") == 2
    g.set_receivers(np.zeros((256, 3)), np.full(256, 0.5))
    assert g.get_option("receivers") == 256
    P = T.Polygon_Count
    for top, alpha in [(1, np.zeros((P, 2))), (-1, np.zeros((P, 2))), (0, np.zeros((P, 9))), (0, np.full((P, 2), -0.01)),
                       (0, np.full((P, 2), 1.01)), (0, np.full((P, 2), np.nan))]:
        with pytest.raises(H.HareError) as ei:
            g.set_absorption(alpha, top)
        assert ei.value.code == capi.HARE_E_INVALID
    rc = capi.lib.hare_scene_set_absorption(g._h, 0, 0, capi.ptr(np.zeros(P)))
    assert rc == capi.HARE_E_INVALID
    assert g.get_option("bands") == 1
    a = np.zeros((P, 8))
    a[:, 3] = 1.0
    g.set_absorption(a)
    assert g.get_option("bands") == 8
    g.set_option("receive_aggregate", 0)
    assert g.get_option("receive_aggregate") == 0


def batch_rc(g, n=8, bounces=3, n_bins=10, bin_len=0.01, frac_bits=40, rays=True, hist=True, det=True, top=0, kind=None):
    r = np.zeros((min(max(n, 1), 64), 6))         # never read: every case is refused first
    h = np.zeros(1 << 16, np.uint64)
    d = np.zeros(1024, np.uint64)
    return capi.lib.hare_receive_batch(g._h, g._kind if kind is None else kind, top, n, capi.ptr(r) if rays else None, None, None, bounces, 0,
                                       n_bins, bin_len, frac_bits, None, None, capi.ptr(h) if hist else None, capi.ptr(d) if det else None, None)


def test_bad_receive_arguments_are_invalid_before_anything_runs():
    g, _ = grid()
    g.set_receivers([[1.0, 1.0, 1.0]], [0.5])
    E = capi.HARE_E_INVALID
    for kw in [dict(n_bins=0), dict(n_bins=-5), dict(bin_len=0.0), dict(bin_len=-1.0), dict(bin_len=np.inf), dict(bin_len=np.nan),
               dict(frac_bits=-1), dict(frac_bits=63), dict(bounces=0), dict(bounces=4097), dict(n=-1), dict(n=0x7FFFFF01),
               dict(n_bins=(1 << 27) + 1), dict(rays=False), dict(hist=False), dict(det=False), dict(top=1), dict(kind=3)]:
        assert batch_rc(g, **kw) == E, kw
    g.set_receivers(np.zeros((8, 3)), np.ones(8))
    g.set_absorption(np.zeros((g.Model[0].Polygon_Count, 8)))
    assert batch_rc(g, n_bins=(1 << 21) + 1) == E                     # 8 x 2^21 x 8 > 2^27
    # the device call: the same checks, and overlapping buffers (addresses are never touched before the checks pass)
    lib = capi.lib
    n = 1000
    base = 1 << 40

    def dev(**kw):
        a = dict(rays=base, state=base + (1 << 30), work=base + (2 << 30), ev=base + (3 << 30), hist=base + (4 << 30), det=base + (5 << 30),
                 ctr=None, e1=None, n_bins=10, bin_len=0.5, frac_bits=30, n=n)
        a.update(kw)
        return lib.hare_receive_device(g._h, g._kind, 0, a["n"], a["rays"], a["e1"], None, 4, 0, a["n_bins"], a["bin_len"], a["frac_bits"],
                                       a["state"], a["work"], a["ev"], a["hist"], a["det"], a["ctr"], None)
    for kw in [dict(state=base + 48 * n - 8), dict(work=base + (1 << 30) + 8), dict(ev=base + (2 << 30)), dict(hist=base + (3 << 30) + 56 * n - 8),
               dict(det=base + (4 << 30) + 8), dict(ctr=base + (5 << 30) + 8), dict(e1=base + (2 << 30) + 4), dict(state=None), dict(hist=None),
               dict(n_bins=0), dict(bin_len=np.inf), dict(frac_bits=99)]:
        assert dev(**kw) == E, kw


def test_a_receive_call_without_a_gpu_is_nodevice_and_without_receivers_is_state(gpu_available):
    g, _ = grid()
    rays = H.scenes.burst_rays(64, H.scenes.shoebox().size)
    with pytest.raises(H.HareError) as ei:
        g.Receive_batch(rays, 4, 100, 0.01)
    assert ei.value.code == (capi.HARE_E_STATE if gpu_available else capi.HARE_E_NODEVICE)      # no receivers yet: STATE on a GPU
    g.set_receivers([[1.0, 1.0, 1.0]], [0.5])
    if not gpu_available:
        with pytest.raises(H.HareError) as ei:
            g.Receive_batch(rays, 4, 100, 0.01)
        assert ei.value.code == capi.HARE_E_NODEVICE
        rc = capi.lib.hare_receive_device(g._h, g._kind, 0, 16, 1 << 40, None, None, 4, 0, 10, 0.5, 30, 2 << 40, 3 << 40, 4 << 40, 5 << 40,
                                          6 << 40, None, None)
        assert rc == capi.HARE_E_NODEVICE


# ---- the restatement on hand-worked cases
def step(o, d, t_end, L=0.0, E=(1.0,), c=(0.0, 0.0, 0.0), r=1.0, n_bins=10, bin_len=1.0, frac_bits=0, K=1):
    B = len(E)
    hist = np.zeros((K, n_bins, B), np.uint64)
    det = np.zeros((K, 2), np.uint64)
    receiver_step(np.array([o], float), np.array([d], float), np.array([t_end], float), np.array([L], float), np.array(E, float).reshape(B, 1),
                  np.array([c], float), np.array([r], float), n_bins, bin_len, frac_bits, hist, det)
    return hist, det


def test_restatement_ray_through_the_center():
    hist, det = step((-5.0, 0, 0), (1.0, 0, 0), np.inf, L=2.0, E=(0.5, 0.25), frac_bits=4)
    # s = 5, x = (2 + 5) / 1 = 7 -> bin 7; q = 0.5 * 16 = 8, 0.25 * 16 = 4
    assert det.tolist() == [[1, 0]]
    assert hist[0, 7].tolist() == [8, 4] and int(hist.sum()) == 12


def test_restatement_exact_tangent_is_not_detected():
    hist, det = step((-5.0, 1.0, 0), (1.0, 0, 0), np.inf)       # closest distance^2 = 1 = r*r: strict <
    assert det.tolist() == [[0, 0]] and int(hist.sum()) == 0
    hist, det = step((-5.0, 0.9990234375, 0), (1.0, 0, 0), np.inf)
    assert det.tolist() == [[1, 0]]


def test_restatement_s_exactly_at_t_end_and_behind_the_origin():
    assert step((-5.0, 0, 0), (1.0, 0, 0), 5.0)[1].tolist() == [[0, 0]]           # s == t_end: the wall comes first
    assert step((-5.0, 0, 0), (1.0, 0, 0), 5.0000000000000009)[1].tolist() == [[1, 0]]
    assert step((5.0, 0, 0), (1.0, 0, 0), np.inf)[1].tolist() == [[0, 0]]         # s < 0
    assert step((0.0, 0, 0), (1.0, 0, 0), np.inf)[1].tolist() == [[1, 0]]         # s == 0 (origin at the center) counts
    assert step((-5.0, 0, 0), (0.0, 0, 0), np.inf)[1].tolist() == [[0, 0]]        # zero direction: s is NaN


def test_restatement_bin_edges():
    # x = (L + 5) / 0.5: L = -5 -> x = 0 -> bin 0; L = 0 -> x = 10 = n_bins -> not binned (counted in detections[2k+1]); L = -5.5 -> x < 0
    hist, det = step((-5.0, 0, 0), (1.0, 0, 0), np.inf, L=-5.0, bin_len=0.5, frac_bits=1)
    assert det.tolist() == [[1, 0]] and hist[0, 0, 0] == 2
    L = np.nextafter(4.5, 0.0) - 5.0                                      # exact: L + 5 is the double just below 4.5
    hist, det = step((-5.0, 0, 0), (1.0, 0, 0), np.inf, L=L, bin_len=0.5, frac_bits=1, n_bins=10)
    assert det.tolist() == [[1, 0]] and hist[0, 8, 0] == 2              # x = 8.999999999999998 -> bin 8
    for L in (0.0, -5.5):
        hist, det = step((-5.0, 0, 0), (1.0, 0, 0), np.inf, L=L, bin_len=0.5)
        assert det.tolist() == [[0, 1]] and int(hist.sum()) == 0


def test_restatement_quantisation_saturation_and_wrap():
    assert quantise([0.5, 1.5, 2.5, -1.0, np.nan, 0.0, -0.0], 0).tolist() == [0, 2, 2, 0, 0, 0, 0]          # rint: half to even
    assert quantise([np.inf, 1e300, 2.0], 62).tolist() == [1 << 63, 1 << 63, 1 << 63]                      # min(q, 2^63)
    assert quantise([1.0], 62).tolist() == [1 << 62]
    hist = np.zeros((1, 1, 1), np.uint64)
    det = np.zeros((1, 2), np.uint64)
    o = np.array([[-5.0, 0, 0]] * 3)
    d = np.array([[1.0, 0, 0]] * 3)
    receiver_step(o, d, np.full(3, np.inf), np.zeros(3), np.full((1, 3), 1.0), [[0.0, 0, 0]], [1.0], 1, 100.0, 62, hist, det)
    assert int(hist[0, 0, 0]) == (3 << 62) % (1 << 64) and det.tolist() == [[3, 0]]                          # wraps mod 2^64


def test_bands_are_read_per_topology_whoever_set_the_table():
    m = H.scenes.shoebox()
    T0, T1 = H.Topology(m.verts, m.nverts), H.Topology(m.verts, m.nverts)
    g = H.Voxel_Grid([T0, T1], 8)
    P = T1.Polygon_Count
    a = np.full((P, 8), 0.5)
    assert capi.lib.hare_scene_set_absorption(g._h, 1, 8, capi.ptr(a)) == capi.HARE_OK      # not through this object's set_absorption
    assert g.get_option("bands") == 1 and g.get_option("bands:0") == 1 and g.get_option("bands:1") == 8
    assert g._bands(1) == 8 and g._bands(0) == 1
    for bad in ("bands:2", "bands:-1", "bands:", "bands:1x"):
        with pytest.raises(H.HareError) as ei:
            g.get_option(bad)
        assert ei.value.code == capi.HARE_E_INVALID
