"""First-order image sources on the CPU (include/hare_hip.h, "receivers", "Image sources (first order)"): that the device cases of
tests/test_gpu_image.py hold every class of the definition (counted with tests/image_ref.py alone, so that the device tests cannot pass
vacuously); that n * sum_p f(k, p) is the number of a burst's rays that the sampled loop detects in cast 1 -- the one thing a byte
comparison cannot see, as reference and kernel share the formula; that the suppression rule restated on the reference loop obeys the
header's identity; and the refusals and the check order of hare_image_device and of HARE_RECEIVE_IMAGE on every receive call."""
import collections
import ctypes as C

import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from oracle import pyoracle as po
from tests import image_ref as ir
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
    return {c.name: (c, ir.reference(c)) for c in ir.cases()}


def test_cases_span_the_axes():
    cs = ir.cases()
    assert {c.partition[0] for c in cs} == {"voxel", "octree", "kdtree"} and {c.scene for c in cs} == {"box12", "box972", "quads", "baffle"}
    assert {(c.scene, c.partition[0]) for c in cs} >= {(s, p) for s in ("box972", "quads", "baffle") for p in ("voxel", "octree", "kdtree")}
    assert {c.K for c in cs if not c.map} == {1, 3, 64, 65, 256} and {c.K for c in cs if c.map} == {257}
    P = {ir.mesh_of(c.scene)[0].shape[0] for c in cs}
    assert P == {12, 54, 56, 972} and all(p % 64 and p % 256 for p in P) and max(P) > 256          # no multiple of the wave or the tile; several blocks
    assert {c.B for c in cs} == {1, 3, 8} and {c.R for c in cs} == {0, 4} and {c.frac_bits for c in cs} == {0, 40, 62}
    assert {c.tables for c in cs} >= {"alpha", "alpha+sigma"}
    assert 1 in {c.n_bins for c in cs} and max(c.n_bins for c in cs) >= 256 and {c.directional for c in cs} == {False, True}
    assert {c.n_weight for c in cs} == {1, 4097, 2 ** 40}
    assert (ir.mesh_of("quads")[1] == 4).all() and (ir.mesh_of("box972")[1] == 3).all()


def multiplicity(seen):
    """How many accepted pairs share a receiver and a reflection point, at most."""
    cnt = collections.Counter((int(k), x.tobytes()) for k, x in zip(seen["k"], seen["x"]))
    return max(cnt.values()) if cnt else 0


def test_cases_hold_every_class_of_the_definition(references):
    some = lambda f: [n for n, (c, r) in references.items() if f(c, r)]
    s_ = lambda r: r["seen"]
    assert some(lambda c, r: s_(r)["unmirrored"].any())                                       # a source on a polygon's plane, h == 0
    assert (references["baffle-K64-h0"][1]["seen"]["h"] == 0).sum() == 8
    assert some(lambda c, r: s_(r)["ineligible"] > 0)                                         # the image inside a receiver's sphere
    assert some(lambda c, r: s_(r)["behind"] > 0)                                             # a receiver behind the plane
    assert some(lambda c, r: multiplicity(s_(r)) == 2) and some(lambda c, r: multiplicity(s_(r)) == 6)   # a shared edge; a corner
    assert some(lambda c, r: (s_(r)["edge"] & s_(r)["binned"]).any())                         # a path length on a bin edge ...
    at_end = some(lambda c, r: (s_(r)["edge"] & ~s_(r)["binned"] & ~s_(r)["occ_rcv"] & ~s_(r)["occ_src"]).any() and c.n_bins * c.bin_len == 6.0)
    assert at_end == ["box12-K3-dir"]                                                         # ... and at n_bins
    assert some(lambda c, r: r["pairs"] == 0) == ["box12-K1-none"]                            # zero accepted pairs
    for legs in ((True, False), (False, True), (True, True), (False, False)):                 # blocked on the receiver's leg, the source's, both, neither
        assert some(lambda c, r: c.scene == "baffle" and ((s_(r)["occ_rcv"] == legs[0]) & (s_(r)["occ_src"] == legs[1])).any()), legs
    assert some(lambda c, r: c.frac_bits == 62 and r["tallies"].get("saturated", 0) > 0)
    assert some(lambda c, r: r["tallies"].get("round_to_zero", 0) > 0) and some(lambda c, r: r["tallies"].get("wrapped", 0) > 0)
    assert some(lambda c, r: c.directional and r["tallies"].get("dir_clamped", 0) > 0)
    faces = set()
    for c, r in references.values():
        faces |= r["seen"]["faces"]
    assert len(faces) >= 5
    for name, (c, r) in references.items():                          # detections count the pairs with both legs free, each once
        s = r["seen"]
        free = ~s["occ_rcv"] & ~s["occ_src"]
        assert int(r["det"].sum()) == int(free.sum()) and int(r["det"][:, 0].sum()) == int(s["binned"].sum()), name
        assert r["pairs"] == s["k"].size and (r["pairs"] > 0 or c.big), name
        if not c.big and c.scene != "baffle":
            assert r["pairs"] >= 6 * c.K - 2, name                    # a closed box: a path via every wall, but for the ineligible ones


# ---- (b) the scale of n * sum_p f(k, p)
SEEDS = (0, 11, 2024)
N_BURST = 65536


def cone_inside_wall(S, c, r, axis, plane, size):
    """The cone from the image S that touches the sphere (c, r) meets the wall `axis` = plane wholly inside the wall's rectangle."""
    v = c - S
    dist = np.linalg.norm(v)
    w = v / dist
    e1 = np.cross(w, [1.0, 0.3, 0.2])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(w, e1)
    sin = r / dist
    phi = np.linspace(0, 2 * np.pi, 256, endpoint=False)
    d = np.sqrt(1 - sin * sin) * w[None] + sin * (np.cos(phi)[:, None] * e1[None] + np.sin(phi)[:, None] * e2[None])
    t = (plane - S[axis]) / d[:, axis]
    x = S[None] + d * t[:, None]
    other = [a for a in range(3) if a != axis]
    return bool((t > 0).all() and all((x[:, a] > 0.05).all() and (x[:, a] < size[a] - 0.05).all() for a in other))


def test_the_deposit_is_the_expected_count_of_cast_1():
    """Four receivers in the 12-triangle shoebox, wholly inside it, whose six first-order cones no wall edge clips (checked here: every
    cone's footprint lies inside its wall).  The reference loop's cast-1 detections of three 65 536-ray bursts, receiver by receiver,
    against n * sum_p f(k, p) over the valid images: within 4.5 sigma of the binomial (12 pairs; a factor wrong misses by tens of sigma)."""
    verts, nverts, size = ir.mesh_of("box12")
    To, o, normals = ir.oracle_of("box12", ir.PARTITIONS[0])
    pos = np.array([4.0, 3.0, 1.75])
    centers = np.array([[6.5, 4.0, 2.25], [3.0, 4.25, 1.5], [5.5, 2.5, 2.0], [2.75, 2.5, 2.25]])
    radii = np.array([0.5, 0.45, 0.55, 0.4])
    assert ((centers - radii[:, None] > 0) & (centers + radii[:, None] < np.asarray(size))).all()
    f = ir.pairs(pos, verts, nverts, normals, centers, radii)
    assert f["k"].size == 6 * 4 and multiplicity(f) == 1 and f["ineligible"] == 0            # one triangle per wall and receiver
    for k, p, S in zip(f["k"], f["p"], f["S"][f["p"]]):
        axis = int(np.argmax(np.abs(normals[p])))
        assert cone_inside_wall(S, centers[k], radii[k], axis, verts[p, 0, axis], size), (k, p)
    # both legs free in a convex room
    hist, det = np.zeros((4, 1, 1), np.uint64), np.zeros((4, 2), np.uint64)
    assert ir.image(o, verts, nverts, normals, pos, [1.0], None, 0, None, None, None, centers, radii, 1, 1, 100.0, 0, hist, det) == 24
    assert (det[:, 0] == 6).all()
    F = np.zeros(4)
    np.add.at(F, f["k"], ir.share((radii * radii)[f["k"]], f["d2"]))
    assert (F > 0.004).all() and (F < 0.05).all()
    for seed in SEEDS:
        rays, state = sr.emit(seed, 0, N_BURST, pos, [1.0], None, 0, None)
        two = rr.receive_loop(po, To, o, rays, 2, centers, radii, 1, 100.0, 0, state_in=state)[1]
        one = rr.receive_loop(po, To, o, rays, 1, centers, radii, 1, 100.0, 0, state_in=state)[1]
        count = (two - one).sum(axis=1).astype(np.float64)
        sigma = np.sqrt(N_BURST * F * (1 - F))
        print(seed, count, np.round(N_BURST * F, 1), np.round((count - N_BURST * F) / sigma, 2))
        assert (np.abs(count - N_BURST * F) <= 4.5 * sigma).all(), (seed, count, N_BURST * F)


# ---- (c) the suppression rule on the reference loop
def test_the_suppressed_reference_obeys_the_identity_without_a_table_and_splits_the_rays_with_one():
    verts, nverts, size = ir.mesh_of("baffle")
    To, o, normals = ir.oracle_of("baffle", ir.PARTITIONS[0])
    c = ir.ImageCase("s", "baffle", ir.PARTITIONS[0], 6, False, 3, 0, "alpha+sigma", 30, 32, 0.5, False, 1, pos=(2.0, 1.0, 1.0))
    centers, radii = c.receivers()
    alpha, sigma = c.absorption()
    rays, state = sr.emit(3, 0, 4097, np.array(c.pos), sr.powers(3), None, 0, None)
    loop = lambda b, sg: rr.receive_loop(po, To, o, rays, b, centers, radii, 32, 0.5, 30, alpha=alpha, sigma=sg, seed=5, state_in=state)
    for b in (2, 5):
        h, d, st, split = ir.suppressed(To, o, rays, state, b, centers, radii, 32, 0.5, 30, alpha=alpha)
        with np.errstate(over="ignore"):
            assert (h == loop(b, None)[0] - loop(2, None)[0] + loop(1, None)[0]).all() and (d == loop(b, None)[1] - loop(2, None)[1] + loop(1, None)[1]).all()
        assert split["diffuse"] == 0 and split["specular"] > 4000 and st.tobytes() == loop(b, None)[2].tobytes()
        h, d, st, split = ir.suppressed(To, o, rays, state, b, centers, radii, 32, 0.5, 30, alpha=alpha, sigma=sigma, seed=5)
        plain = loop(b, sigma)
        assert split["diffuse"] > 500 and split["specular"] > 500 and st.tobytes() == plain[2].tobytes()
        assert (d <= plain[1]).all() and (d != plain[1]).any() and (h <= plain[0]).all()          # something, but not everything, of cast 1 is gone
        with np.errstate(over="ignore"):
            gone = plain[1] - d
        assert 0 < int(gone.sum()) < int((loop(2, sigma)[1] - loop(1, sigma)[1]).sum()) or b > 2
    h1 = ir.suppressed(To, o, rays, state, 1, centers, radii, 32, 0.5, 30, alpha=alpha, sigma=sigma, seed=5)[0]
    assert (h1 == loop(1, sigma)[0]).all()                               # one cast: nothing is suppressed


# ---- (d) refusals and check order
def grid():
    m = H.scenes.shoebox()
    return H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8), m


def test_image_device_checks_in_order(gpu_available):
    g, m = grid()
    lib, h = capi.lib, g._h
    W, HI, D = 1 << 20, 2 << 20, 3 << 20                                # addresses are only compared before a device is found

    def call(n_weight=5, n_bins=8, bin_len=0.5, frac_bits=20, max_pairs=4, work=W, hist=HI, det=D, kind=capi.KIND_VOXEL, top=0, flags=0):
        return lib.hare_image_device(h, kind, top, n_weight, flags, n_bins, bin_len, frac_bits, max_pairs, work, hist, det, None)
    for bad in (dict(n_weight=0), dict(n_weight=-1), dict(n_weight=2 ** 53 + 1), dict(n_bins=0), dict(bin_len=0.0), dict(bin_len=float("nan")),
                dict(frac_bits=-1), dict(frac_bits=63), dict(kind=7), dict(top=1), dict(n_bins=2 ** 27 + 1), dict(n_bins=2 ** 25 + 1, flags=256),
                dict(max_pairs=0), dict(max_pairs=-3), dict(max_pairs=2 ** 26 + 1), dict(work=None), dict(hist=None), dict(det=None),
                dict(work=W + 8), dict(hist=W + 64), dict(det=W + 300), dict(det=HI + 8)):
        assert call(**bad) == E_INVALID, bad
    wb = H.Voxel_Grid.image_work_bytes(1, 972, 4)
    assert wb == 256 + 32 * 972 + 136 * 4
    assert call(hist=W + wb - 8) == E_INVALID and "overlap" in capi.last_error()
    assert call(n_weight=2 ** 53, hist=W + wb, det=W + wb + 64) == (E_STATE if gpu_available else E_NODEVICE)
    g.set_receivers([np.asarray(m.size) * 0.5] * 2, [0.5, 0.25])
    assert call(det=HI + 2 * 8 * 8 - 8) == E_INVALID                   # sizes follow K
    assert call() == (E_STATE if gpu_available else E_NODEVICE)
    if gpu_available:
        assert "no source" in capi.last_error()
    g.set_source(np.asarray(m.size) * 0.3, power=np.ones(3))
    assert call() == E_INVALID and "bands" in capi.last_error()         # before any device is looked for
    assert call(max_pairs=0) == E_INVALID and "bands" in capi.last_error()      # ... and before max_pairs
    g.set_absorption(np.full((g.Model[0].Polygon_Count, 3), 0.1))
    if not gpu_available:
        assert call() == E_NODEVICE


def test_the_flag_is_refused_on_the_batch_calls_and_checked_in_order_on_the_others(gpu_available):
    g, m = grid()
    g.set_receivers([np.asarray(m.size) * 0.5], [0.5])
    rays = H.scenes.random_rays(8, m.size)
    lib, h = capi.lib, g._h
    FLAG = capi.RECEIVE_IMAGE
    assert FLAG == 2048 and FLAG < 0x1000 and FLAG == 2 * capi.RECEIVE_DIRECT          # the next free bit, below the developer bits
    hist, det, ctr = np.zeros(10, np.uint64), np.zeros(2, np.uint64), capi.Counters()
    batch = lambda flags: lib.hare_receive_batch(h, g._kind, 0, 8, capi.ptr(rays), None, None, 2, flags, 10, 0.1, 20, None, None, capi.ptr(hist),
                                                 capi.ptr(det), C.addressof(ctr))
    assert batch(FLAG) == E_INVALID and "HARE_RECEIVE_IMAGE" in capi.last_error()
    assert batch(FLAG | capi.RECEIVE_DIRECT) == E_INVALID and batch(FLAG | capi.RECEIVE_DIRECTIONAL) == E_INVALID
    handles = (C.c_void_p * 1)(h)
    assert lib.hare_receive_batch_sharded(handles, 1, g._kind, 0, 8, capi.ptr(rays), None, None, 2, FLAG, 10, 0.1, 20, None, None, capi.ptr(hist),
                                          capi.ptr(det), C.addressof(ctr)) == E_INVALID
    sums, win = np.zeros(4, np.uint64), np.array([0, 10], np.int32)
    assert lib.hare_receive_batch_reduced(h, g._kind, 0, 8, capi.ptr(rays), None, None, 2, FLAG, 10, 0.1, 20, None, None, None, 1, capi.ptr(win), 0,
                                          None, capi.ptr(sums), None, capi.ptr(det), C.addressof(ctr)) == E_INVALID
    if not gpu_available:
        assert batch(0) == E_NODEVICE                                                  # nothing else about the call has moved
    # the source calls: their own checks first, then the device, then the state (no source)
    assert code(lambda: g.Receive_source(16, 2, 10, 0.0, image=True)) == E_INVALID
    assert code(lambda: g.Receive_source(16, 2, 10, 0.1, image=True)) == (E_STATE if gpu_available else E_NODEVICE)
    assert code(lambda: g.Receive_source_reduced(16, 2, 10, 0.1, windows=[(0, 10)], image=True, direct=True)) == (E_STATE if gpu_available else E_NODEVICE)
    if gpu_available:
        assert "no source" in capi.last_error()
    dev = lambda: g.receive_device(8, 1 << 20, 2, 10, 0.1, 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20, image=True)
    assert code(dev) == (E_STATE if gpu_available else E_NODEVICE)
    g.set_source(np.asarray(m.size) * 0.3, power=np.ones(3))
    assert code(lambda: g.Receive_source(16, 2, 10, 0.1, image=True)) == E_INVALID and "bands" in capi.last_error()
    assert code(dev) == E_INVALID and "bands" in capi.last_error()
    # the options of the host calls' pair list and of the A/B
    assert g.get_option("image_max_pairs") == 1 << 20 and g.get_option("image_cull") == 1
    assert code(lambda: g.set_option("image_max_pairs", 0)) == E_INVALID and code(lambda: g.set_option("image_cull", 2)) == E_INVALID
    g.set_option("image_max_pairs", 7).set_option("image_cull", 0)
    assert g.get_option("image_max_pairs") == 7 and g.get_option("image_cull") == 0
