"""Second-order image sources on the CPU (include/hare_hip.h, "receivers", "Image sources (second order)"): that the device cases of
tests/test_gpu_image2.py hold the classes of the definition (counted with tests/image2_ref.py alone, so that the device tests cannot pass
vacuously); that the suppression rule restated on the reference loop obeys the header's identity; and the refusals, in order."""
import collections

import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from oracle import pyoracle as po
from tests import image2_ref as i2
from tests import image_ref as ir
from tests import receive_ref as rr
from tests import source_ref as sr
from tests.test_image_ref import code, grid

E_INVALID, E_NODEVICE, E_STATE = capi.HARE_E_INVALID, capi.HARE_E_NODEVICE, capi.HARE_E_STATE


@pytest.fixture(scope="module")
def references():
    return {c.name: (c, i2.reference(c)) for c in i2.cases()}


def multiplicity(seen):
    """How many accepted paths share a receiver and both reflection points, at most."""
    cnt = collections.Counter((int(k), a.tobytes(), b.tobytes()) for k, a, b in zip(seen["k"], seen["x1"], seen["x2"]))
    return max(cnt.values()) if cnt else 0


def test_cases_hold_the_classes_of_the_definition(references):
    some = lambda f: [n for n, (c, r) in references.items() if f(c, r)]
    s_ = lambda r: r["seen"]
    cs = i2.cases()
    assert {c.partition[0] for c in cs} == {"voxel", "octree", "kdtree"} and {ir.mesh_of(c.scene)[0].shape[0] for c in cs} == {3, 12, 54, 56, 972}
    assert {c.K for c in cs if not c.map} == {1, 8, 256} and {c.K for c in cs if c.map} == {257} and {c.directional for c in cs} == {False, True}
    assert some(lambda c, r: s_(r)["cands"]["h2_zero"] > 0)                                    # h2 == 0: no second image
    assert all((s_(r)["cands"]["same"] > 0 or c.scene == "corner3") and (s_(r)["cands"]["p"] != s_(r)["cands"]["q"]).all()
               for c, r in references.values())                                                # p == q skipped
    assert some(lambda c, r: s_(r)["ineligible"] > 0)                                          # a second image inside a sphere
    for legs in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)):                                  # each leg blocked alone, and none
        assert some(lambda c, r: r["paths"] and (s_(r)["occ"] == np.array(legs, bool)).all(axis=1).any()), legs
    assert some(lambda c, r: multiplicity(s_(r)) >= 2)                                         # a path through a shared edge
    assert some(lambda c, r: r["paths"] and (s_(r)["edge"] & s_(r)["binned"]).any())           # a path length on a bin edge ...
    assert some(lambda c, r: r["paths"] and (s_(r)["edge"] & ~s_(r)["binned"] & ~s_(r)["occ"].any(axis=1)).any())      # ... and at n_bins
    assert some(lambda c, r: r["cands"] == 0) == ["corner3-K8-nocands"]                        # zero candidates: no polygon mirrors the source
    assert s_(references["corner3-K8-nocands"][1])["cands"]["unmirrored"].all()
    assert some(lambda c, r: r["paths"] == 0 and r["cands"] > 0) == ["box12-K1-none"]          # zero paths among 132 candidates
    quads = [r for c, r in references.values() if c.scene == "quads"]
    assert quads and all(r["paths"] > 0 for r in quads) and (ir.mesh_of("quads")[1] == 4).all()  # a quadrilateral as p and as q
    for name, (c, r) in references.items():
        s = r["seen"]
        if r["paths"]:
            assert int(r["det"].sum()) == int((~s["occ"].any(axis=1)).sum()) and int(r["det"][:, 0].sum()) == int(s["binned"].sum()), name


def test_the_suppressed_reference_obeys_the_identity_without_a_table_and_splits_the_rays_with_one():
    To, o, normals = ir.oracle_of("baffle", ir.PARTITIONS[0])
    c = i2.Image2Case("s", "baffle", ir.PARTITIONS[0], 6, False, 3, 0, "alpha+sigma", 30, 32, 0.5, False, 1, pos=(2.0, 1.0, 1.0))
    centers, radii = c.receivers()
    alpha, sigma = c.absorption()
    rays, state = sr.emit(3, 0, 4097, np.array(c.pos), sr.powers(3), None, 0, None)
    loop = lambda b, sg: rr.receive_loop(po, To, o, rays, b, centers, radii, 32, 0.5, 30, alpha=alpha, sigma=sg, seed=5, state_in=state)
    for b in (3, 5):
        h, d, st, split = i2.suppressed2(To, o, rays, state, b, centers, radii, 32, 0.5, 30, alpha=alpha)
        with np.errstate(over="ignore"):
            assert (h == loop(b, None)[0] - loop(3, None)[0] + loop(1, None)[0]).all() and (d == loop(b, None)[1] - loop(3, None)[1] + loop(1, None)[1]).all()
        assert split["other"] == 0 and split["twice"] > 3500 and st.tobytes() == loop(b, None)[2].tobytes()
        h, d, st, split = i2.suppressed2(To, o, rays, state, b, centers, radii, 32, 0.5, 30, alpha=alpha, sigma=sigma, seed=5)
        first = ir.suppressed(To, o, rays, state, b, centers, radii, 32, 0.5, 30, alpha=alpha, sigma=sigma, seed=5)
        assert split["twice"] > 300 and split["other"] > 300 and st.tobytes() == loop(b, sigma)[2].tobytes()
        assert (d <= first[1]).all() and (d != first[1]).any() and (h <= first[0]).all()      # something more than the first order takes is gone
    for b in (1, 2):                                                    # nothing more is suppressed
        assert (i2.suppressed2(To, o, rays, state, b, centers, radii, 32, 0.5, 30, alpha=alpha, sigma=sigma, seed=5)[0] ==
                ir.suppressed(To, o, rays, state, b, centers, radii, 32, 0.5, 30, alpha=alpha, sigma=sigma, seed=5)[0]).all()


def test_the_flag_and_the_entry_point_check_in_order(gpu_available):
    g, m = grid()
    g.set_receivers([np.asarray(m.size) * 0.5], [0.5])
    lib, h = capi.lib, g._h
    FLAG = capi.RECEIVE_IMAGE2
    assert FLAG == 0x10000 and FLAG & (0xF000 | 0x40000 | 0x80000) == 0 and FLAG & (FLAG - 1) == 0
    # alone: refused first, whatever else is wrong with the call
    assert code(lambda: g.Receive_source(16, 3, 10, 0.0, image2=True)) == E_INVALID and "HARE_RECEIVE_IMAGE2" in capi.last_error()
    assert code(lambda: g.Receive_source(16, 3, 10, 0.1, image2=True, direct=True)) == E_INVALID and "HARE_RECEIVE_IMAGE2" in capi.last_error()
    # with the first-order flag: the call's own checks, then the device, then the state (no source)
    assert code(lambda: g.Receive_source(16, 3, 10, 0.0, image=True, image2=True)) == E_INVALID
    assert code(lambda: g.Receive_source(16, 3, 10, 0.1, image=True, image2=True)) == (E_STATE if gpu_available else E_NODEVICE)
    rays = H.scenes.random_rays(8, m.size)
    hist, det, ctr = np.zeros(10, np.uint64), np.zeros(2, np.uint64), capi.Counters()
    import ctypes as C
    batch = lambda flags: lib.hare_receive_batch(h, g._kind, 0, 8, capi.ptr(rays), None, None, 3, flags, 10, 0.1, 20, None, None, capi.ptr(hist),
                                                 capi.ptr(det), C.addressof(ctr))
    assert batch(FLAG | capi.RECEIVE_IMAGE) == E_INVALID and batch(FLAG) == E_INVALID
    W, HI, D = 1 << 20, 2 << 20, 3 << 20

    def call(n_weight=5, n_bins=8, bin_len=0.5, frac_bits=20, max_cands=4, max_paths=4, work=W, hist=HI, det=D, kind=capi.KIND_VOXEL, top=0, flags=0):
        return lib.hare_image2_device(h, kind, top, n_weight, flags, n_bins, bin_len, frac_bits, max_cands, max_paths, work, hist, det, None)
    for bad in (dict(n_weight=0), dict(n_weight=2 ** 53 + 1), dict(n_bins=0), dict(bin_len=0.0), dict(frac_bits=63), dict(kind=7), dict(top=1),
                dict(max_cands=0), dict(max_paths=0), dict(max_cands=2 ** 26 + 1), dict(max_paths=2 ** 26 + 1), dict(work=None), dict(hist=None),
                dict(det=None), dict(work=W + 8), dict(hist=W + 64)):
        assert call(**bad) == E_INVALID, bad
    wb = H.Voxel_Grid.image2_work_bytes(972, 4, 4)
    assert wb == 256 + 32 * 972 + 32 * 4 + 212 * 4
    assert call(hist=W + wb - 8) == E_INVALID and "overlap" in capi.last_error()
    assert call(hist=W + wb, det=W + wb + 128) == (E_STATE if gpu_available else E_NODEVICE)
    assert H.Voxel_Grid.receive_work_bytes(100, image2=True) == 900 and H.Voxel_Grid.receive_work_bytes(100, rain=True, image2=True) == 8356
    assert g.get_option("image2_max_cands") == 1 << 22 and g.get_option("image2_max_paths") == 1 << 20 and g.get_option("image2_prune") == 1
    assert code(lambda: g.set_option("image2_max_cands", 0)) == E_INVALID and code(lambda: g.set_option("image2_prune", 2)) == E_INVALID
    g.set_option("image2_max_cands", 7).set_option("image2_max_paths", 9).set_option("image2_prune", 0)
    assert (g.get_option("image2_max_cands"), g.get_option("image2_max_paths"), g.get_option("image2_prune")) == (7, 9, 0)


# ---- the scale of n * sum f: the definition is the sampled loop's expectation
SEEDS = (0, 11, 2024)
N_BURST = 65536


def cone_clear(S2, S1, c, r, p, q, verts, normals, size, margin=0.05):
    """Every ray of the cone from the second image S2 that touches the sphere (c, r) meets q's wall inside its rectangle and, continued
    from the first image S1, p's wall inside its rectangle between S1 and that point: no edge of either wall clips the cone."""
    v = c - S2
    dist = np.linalg.norm(v)
    w = v / dist
    e1 = np.cross(w, [1.0, 0.3, 0.2])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(w, e1)
    sin = r / dist
    phi = np.linspace(0, 2 * np.pi, 256, endpoint=False)
    d = np.sqrt(1 - sin * sin) * w[None] + sin * (np.cos(phi)[:, None] * e1[None] + np.sin(phi)[:, None] * e2[None])

    def inside(x, axis):
        return all((x[:, a] > margin).all() and (x[:, a] < size[a] - margin).all() for a in range(3) if a != axis)
    aq = int(np.argmax(np.abs(normals[q])))
    t2 = (verts[q, 0, aq] - S2[aq]) / d[:, aq]
    x2 = S2[None] + d * t2[:, None]
    ap = int(np.argmax(np.abs(normals[p])))
    u = x2 - S1[None]
    t1 = (verts[p, 0, ap] - S1[ap]) / u[:, ap]
    x1 = S1[None] + u * t1[:, None]
    return bool((t2 > 0).all() and inside(x2, aq) and (t1 > 0).all() and (t1 < 1).all() and inside(x1, ap))


def test_the_deposit_is_the_expected_count_of_cast_2():
    """Receivers in the 12-triangle shoebox, wholly inside it, each with its 18 second-order paths (six via opposite walls, twelve via
    adjacent ones: of the two orders of an adjacent pair, which share their second image, a receiver is reached by one) and every path's
    cone clear of both walls' edges (checked here), so that no other order of walls carries any ray to them.  The reference loop's
    cast-2 detections of three 65 536-ray bursts, receiver by receiver, against n * sum f over the accepted paths: within 4 sigma of the
    binomial.  The worst deviation observed is recorded in DESIGN.md 7b."""
    verts, nverts, size = ir.mesh_of("box12")
    To, o, normals = ir.oracle_of("box12", ir.PARTITIONS[0])
    pos = np.array([4.0, 3.0, 1.75])
    centers = np.array([[7.25, 3.0, 2.25], [1.75, 4.75, 2.0], [8.25, 4.5, 2.0]])       # found by a search over the room for clear cones
    radii = np.array([0.3, 0.25, 0.3])
    assert ((centers - radii[:, None] > 0) & (centers + radii[:, None] < np.asarray(size))).all()
    f = i2.paths(pos, verts, nverts, normals, centers, radii)
    assert f["k"].size == 18 * 3 and multiplicity(f) == 1 and f["ineligible"] == 0
    cd = f["cands"]
    S2 = {(int(p), int(q)): s for p, q, s in zip(cd["p"], cd["q"], cd["S2"])}
    for k, p, q in zip(f["k"], f["p"], f["q"]):
        assert cone_clear(S2[(int(p), int(q))], cd["S1"][p], centers[k], radii[k], p, q, verts, normals, size), (k, p, q)
    hist, det = np.zeros((3, 1, 1), np.uint64), np.zeros((3, 2), np.uint64)
    assert i2.image2(o, verts, nverts, normals, pos, [1.0], None, 0, None, None, None, centers, radii, 1, 1, 100.0, 0, hist, det)[1] == 54
    assert (det[:, 0] == 18).all()                                    # a convex room: every leg free
    F = np.zeros(3)
    np.add.at(F, f["k"], i2.share((radii * radii)[f["k"]], f["d2"]))
    worst = 0.0
    for seed in SEEDS:
        rays, state = sr.emit(seed, 0, N_BURST, pos, [1.0], None, 0, None)
        three = rr.receive_loop(po, To, o, rays, 3, centers, radii, 1, 100.0, 0, state_in=state)[1]
        two = rr.receive_loop(po, To, o, rays, 2, centers, radii, 1, 100.0, 0, state_in=state)[1]
        count = (three - two).sum(axis=1).astype(np.float64)
        sigma = np.sqrt(N_BURST * F * (1 - F))
        dev = (count - N_BURST * F) / sigma
        worst = max(worst, float(np.abs(dev).max()))
        print(seed, count, np.round(N_BURST * F, 1), np.round(dev, 2))
        assert (np.abs(dev) <= 4.0).all(), (seed, count, N_BURST * F)
    print("worst deviation", round(worst, 2), "sigma")
