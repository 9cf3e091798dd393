"""The source paths' device cases cannot pass vacuously, and their reference is pinned (no GPU).  With tests.path_cases.reference alone:
every edge case holds the class it names -- counted from `seen`, the tallies and the geometry --; every sweep seed deposits something
through at least one order it runs; over the N seeds each order runs in at least a third and finds a free path in at least half of
those; every partition and both values of each option occur.  tests/golden/path_reference_digests.json holds tests.path_cases.digest of
every edge case and sweep seed, so that a later edit of tests/direct_ref.py, tests/image_ref.py or tests/image2_ref.py cannot move the
target unnoticed.  A digest that changes on purpose is a change of the specification: regenerate the file and say so.
The cases at ambisonic orders 2 and 3 (tests.path_cases.ambi_edge_cases, ambi_sweep_case; tests/test_gpu_path_ambi.py) follow below in the
same way, pinned in tests/golden/path_ambi_reference_digests.json: each class is found again in the deposits the reference makes (m and
the arrival vector of each, read where they are handed over) or in the words it returns, and at most a tenth of the sweep's seeds leave the
channels 4 .. C - 1 all zero."""
import numpy as np
import pytest

from tests import ambi_ref
from tests import image2_ref as i2
from tests import image_ref as ir
from tests import path_cases as pc
from tests.receive_ref import magnitude
from tests.test_gpu_path_ambi import N as AMBI_N
from tests.test_gpu_path_sweep import N

EDGES = {c.name: c for c in pc.edge_cases()}


def ref(name):
    return pc.reference(EDGES[name], keep=True)


def geometry(case):
    _, _, normals = pc.oracle_of(case)
    S1, mirrored, h = ir.mirror(case.pos, case.verts, normals)
    return normals, S1, mirrored, h


def test_the_file_holds_exactly_the_cases():
    assert set(pc.pinned_digests()) == {"edge/" + n for n in EDGES} | {f"sweep/{s}" for s in range(N)}


@pytest.mark.parametrize("name", list(EDGES))
def test_edge_case_gives_the_pinned_result(name):
    assert pc.digest(ref(name)) == pc.pinned_digests()["edge/" + name], EDGES[name].describe()


@pytest.mark.parametrize("name", list(EDGES))
def test_edge_case_stands_in_an_oblique_room_where_the_arithmetic_rounds(name):
    """What the axis-aligned cases never had: nn != 1.0 in at least a third of the polygons (the mirror's division rounds), and path
    vectors v = c - S' with a component that does not survive a round trip through float (the pre-cull's conversions round)."""
    case = EDGES[name]
    normals, S1, mirrored, _ = geometry(case)
    nn = ir.dot3(normals[:, 0], normals[:, 1], normals[:, 2], normals[:, 0], normals[:, 1], normals[:, 2])
    assert 3 * int((nn != 1.0).sum()) >= case.P, (int((nn != 1.0).sum()), case.P)
    v = case.centers[:, None, :] - S1[None, mirrored, :]
    assert (v.astype(np.float32).astype(np.float64) != v).any()
    for order, res in ref(name).items():
        assert res["hist"].shape == case.shape and res["det"].shape == (case.K, 2)


@pytest.mark.parametrize("name", [n for n in EDGES if n.startswith("P")])
def test_tile_cases_hold_their_counts(name):
    case, out = EDGES[name], ref(name)
    P = int(name[1:4])
    assert case.P == P and case.K == int(name.split("-")[1][1:]) and case.map == (case.K > 256)
    last = 256 * ((P - 1) // 256)                                       # the first polygon of the last block / tile: 0, 0, 256, 512
    assert P - last == {255: 255, 256: 256, 257: 1, 513: 1}[P]
    if "image2" in out:
        s = out["image2"]["seen"]
        assert out["image2"]["paths"] > 0 and out["image2"]["det"].sum() > 0 and out["image2"]["cands"] > 0.9 * P * (P - 1)
        free = ~s["occ"].any(axis=1)                                    # free paths off the last tile's polygons, as p and as q
        assert (s["p"][free] == P - 1).any() and (s["q"][free] == P - 1).any(), (last, s["p"].max(), s["q"].max())
    else:
        s = out["image"]["seen"]
        assert out["image"]["det"].sum() > 0 and out["direct"]["det"].sum() > 0 and s["occ_rcv"].any() and s["k"].max() == case.K - 1
        assert (s["p"][~s["occ_rcv"] & ~s["occ_src"]] == P - 1).any()     # free pairs off the last block's last polygon


def test_rr_edges_hold_bit_for_bit():
    case, out = EDGES["rr-edges"], ref("rr-edges")
    rr = case.radii * case.radii
    normals, S1, _, _ = geometry(case)
    cd = out["image2"]["seen"]["cands"]
    for j, rel in enumerate((">", "=", "<")):
        for k, origin in ((j, case.pos), (3 + j, S1[case.marks[3 + j][0]]),
                          (6 + j, cd["S2"][np.nonzero((cd["p"] == case.marks[6 + j][0]) & (cd["q"] == case.marks[6 + j][1]))[0][0]])):
            d2 = pc.d2_of(case.centers[k], origin)
            want = {">": np.nextafter(rr[k], np.inf), "=": rr[k], "<": np.nextafter(rr[k], -np.inf)}[rel]
            assert d2 == want, (k, rel, d2, rr[k])
            x = rr[k] / d2
            assert (x < 1.0 and np.sqrt(1.0 - x) < 2e-8) if rel == ">" else x >= 1.0
    d, s1, s2 = out["direct"]["seen"], out["image"]["seen"], out["image2"]["seen"]
    assert d["eligible"][:3].tolist() == [True, False, False] and not d["occluded"][0]
    for k in (3, 4, 5):
        hit = (s1["k"] == k) & (s1["p"] == case.marks[k][0])
        assert hit.sum() == (k == 3) and (k != 3 or (abs(s1["f"][hit] - 0.5) < 1e-7).all() and not (s1["occ_rcv"] | s1["occ_src"])[hit].any())
    for k in (6, 7, 8):
        hit = (s2["k"] == k) & (s2["p"] == case.marks[k][0]) & (s2["q"] == case.marks[k][1])
        assert hit.sum() == (k == 6) and (k != 6 or not s2["occ"][hit].any())
    assert s1["ineligible"] >= 2 and s2["ineligible"] >= 2


def test_the_source_in_and_next_to_an_oblique_plane():
    case = EDGES["source-in-plane"]
    normals, S1, mirrored, h = geometry(case)
    p = case.marks["p"]
    assert h[p] == 0.0 and not mirrored[p] and (np.abs(normals[p]) > 0.05).all()
    near = np.abs(h[48:56]) < 1e-12                                     # the baffle's eight coplanar triangles
    assert near.all() and ((h[48:56] != 0) & mirrored[48:56]).any(), h[48:56]
    out = ref("source-in-plane")
    assert out["image"]["seen"]["unmirrored"][p] and out["image"]["det"].sum() > 0 and out["image2"]["det"].sum() > 0
    case = EDGES["source-ulp-off-plane"]
    normals, S1, mirrored, h = geometry(case)
    assert 0 < abs(h[p]) < 1e-14 and mirrored[p] and np.abs(S1[p] - case.pos).max() < 1e-13
    assert ref("source-ulp-off-plane")["image"]["det"].sum() > 0


def test_coplanar_neighbours_differ_in_bits():
    case = EDGES["coplanar-neighbours"]
    normals, S1, mirrored, h = geometry(case)
    v0 = case.verts[:, 0, :]
    h2 = ir.dot3(S1[:, None, 0] - v0[None, :, 0], S1[:, None, 1] - v0[None, :, 1], S1[:, None, 2] - v0[None, :, 2], normals[None, :, 0],
                 normals[None, :, 1], normals[None, :, 2])                # [p, q], as tests.image2_ref.candidates forms it
    same_wall = (np.abs(normals @ normals.T - 1.0) < 1e-9) & (np.abs(h[None, :] - h[:, None]) < 1e-9) & ~np.eye(case.P, dtype=bool)
    assert same_wall.sum() >= 6 * 17 * 18 // 2
    close = same_wall & (np.abs(h2 + h[None, :]) < 1e-12 * np.abs(h[None, :]))
    assert close.sum() > same_wall.sum() // 2 and (close & (h2 != -h[None, :])).sum() > 20 and (close & (h2 == -h[None, :])).sum() > 0
    assert ref("coplanar-neighbours")["image2"]["det"].sum() > 0


def cone_cosine(case, S1, p):
    corners = case.verts[p, :case.nverts[p]]
    axis = corners.mean(axis=0) - S1[p]
    u = corners - S1[p]
    return (u @ axis / (np.linalg.norm(u, axis=1) * np.linalg.norm(axis))).min()


def test_the_prune_cases_sit_at_its_limits():
    case = EDGES["prune-source-on-wall"]
    normals, S1, mirrored, h = geometry(case)
    assert mirrored[0] and 0.5e-7 < abs(h[0]) < 2e-7 and cone_cosine(case, S1, 0) <= 1e-6
    out = ref("prune-source-on-wall")
    assert (out["image2"]["seen"]["p"] == 0).any() and (out["image2"]["seen"]["q"] == 0).any()
    case = EDGES["prune-small-and-sliver"]
    normals, S1, mirrored, h = geometry(case)
    small, sliver = case.marks["small"], case.marks["sliver"]
    assert cone_cosine(case, S1, small) > 1 - 1e-5                       # a cone of under 5 mrad
    e = case.verts[sliver, :3]
    edges = [np.linalg.norm(e[i] - e[(i + 1) % 3]) for i in range(3)]
    height = np.linalg.norm(np.cross(e[1] - e[0], e[2] - e[0])) / max(edges)
    assert max(edges) / height >= 1000, max(edges) / height
    out = ref("prune-small-and-sliver")
    s1, s2 = out["image"]["seen"], out["image2"]["seen"]
    for k, p in ((0, small), (1, sliver)):
        assert ((s1["k"] == k) & (s1["p"] == p)).any(), (k, p)
    assert (s2["cands"]["p"] == sliver).any() and (s2["cands"]["q"] == sliver).any() and out["image2"]["det"].sum() > 0
    case = EDGES["prune-huge-sphere"]
    c = case.verts[case.marks["huge"], :3]
    rho = np.linalg.norm(c - c.mean(axis=0), axis=1).max()
    room = np.linalg.norm(case.verts[:48, :3].reshape(-1, 3).max(axis=0) - case.verts[:48, :3].reshape(-1, 3).min(axis=0))
    assert np.isfinite(rho) and rho > 300 * room
    assert ref("prune-huge-sphere")["image2"]["det"].sum() > 0


def test_the_prune_margin_case_has_nothing_to_spare():
    """The plane test of the prune as image2.hip states it: kept, since dpl + rho > 0; a sphere 1 % small would be dropped; and the one
    path of (p, q) is free and binned, so dropping the candidate changes the histogram."""
    case, out = EDGES["prune-plane-margin"], ref("prune-plane-margin")
    normals, S1, mirrored, h = geometry(case)
    p, q = case.marks["p"], case.marks["q"]
    corners = case.verts[q, :3]
    g = corners.mean(axis=0)
    rho = np.linalg.norm(corners - g, axis=1).max()
    unit = normals[p] / np.linalg.norm(normals[p])
    dpl = np.sign(h[p]) * np.dot(g - case.verts[p, 0], unit)           # the centroid's distance from p's plane, positive on the source's side
    assert dpl + rho > 1e-3 * rho and dpl + 0.99 * rho < -1e-3 * rho, (dpl, rho)
    s = out["image2"]["seen"]
    at = (s["p"] == p) & (s["q"] == q)
    assert at.sum() == 1 and s["k"][at][0] == 0 and not s["occ"][at].any() and s["binned"][at].all()
    assert 3 * int((np.abs(normals[q]) > 0.05).sum()) == 9              # an oblique nail


def test_the_pre_cull_cases_sit_at_its_limits():
    small, large = ref("cull-scale-1e-3"), ref("cull-scale-1e3")
    assert small["image"]["pairs"] == 0 and small["image2"]["paths"] == 0 and small["direct"]["det"].sum() == 8       # |det| <= 1e-6 everywhere
    assert large["image"]["pairs"] > 40 and large["image2"]["paths"] > 100 and large["image"]["seen"]["occ_rcv"].any()
    assert np.allclose(EDGES["cull-scale-1e-3"].verts * 1e6, EDGES["cull-scale-1e3"].verts)
    case = EDGES["cull-far-from-origin"]
    lo = np.concatenate([case.verts[:, :3].reshape(-1, 3), case.verts[case.nverts == 4, 3]]).min(axis=0)
    out = ref("cull-far-from-origin")
    assert (np.abs(lo) > 9900).all() and out["image"]["det"].sum() > 0 and out["image2"]["det"].sum() > 0
    case = EDGES["cull-grazing-edge"]
    normals, S1, mirrored, h = geometry(case)
    q, p2 = case.marks["q"], case.marks["p2"]
    f = ir.pairs(case.pos, case.verts, case.nverts, normals, case.centers, case.radii)
    cd = i2.candidates(case.pos, case.verts, normals)
    S2 = cd["S2"][np.nonzero((cd["p"] == p2) & (cd["q"] == q))[0][0]]
    s2 = ref("cull-grazing-edge")["image2"]["seen"]
    at = (s2["p"] == p2) & (s2["q"] == q)                               # the whole path: x1 inside p2, every leg free -- the flip reaches the histogram
    assert ((s2["k"] == 2) & at & ~s2["occ"].any(axis=1) & s2["binned"]).sum() == 1 and not ((s2["k"] == 3) & at).any()
    s1 = ref("cull-grazing-edge")["image"]["seen"]
    assert ((s1["k"] == 0) & (s1["p"] == q)).sum() == 1 and not ((s1["k"] == 1) & (s1["p"] == q)).any()
    seen = set()
    for k, (tag, inside) in ((k, m) for k, m in case.marks.items() if isinstance(k, int)):
        if tag == "first":
            got = bool(((f["k"] == k) & (f["p"] == q)).any())
            origin = S1[q]
        else:
            origin = S2
            hit, t = i2.poly_fast_rows(S2[None], (case.centers[k] - S2)[None], case.verts[q][None], case.nverts[q:q + 1], normals[q][None])
            got = bool(hit[0] and 0.0 < t[0] < 1.0)
        assert got == inside, (k, tag, inside)
        seen.add((tag, inside))
    assert seen == {("first", True), ("first", False), ("second", True), ("second", False)}
    for a, b in ((0, 1), (2, 3)):                                        # the two of a pair lie 2e-9 of the segment's length apart
        assert np.linalg.norm(case.centers[a] - case.centers[b]) < 1e-8 * np.linalg.norm(case.centers[a] - case.pos)


@pytest.mark.parametrize("name", ("table-R1-edges", "table-R4-edges"))
def test_the_table_cases_leave_along_the_cube_maps_edges_and_corners(name):
    case, out = EDGES[name], ref(name)
    assert case.R == int(name[7]) and np.abs(case.frame).min() > 1e-3   # a frame with no zero entry
    s1, s2 = out["image"]["seen"], out["image2"]["seen"]
    tags = set()
    for k, (order, tag) in case.marks.items():
        if order == "direct":
            assert out["direct"]["seen"]["binned"][k]
            d = (case.centers[k] - case.pos)[None]
        elif order == "image":
            i = np.nonzero((s1["k"] == k) & s1["binned"])[0]
            d = s1["x"][i] - case.pos[None]
        else:
            i = np.nonzero((s2["k"] == k) & s2["binned"])[0]
            d = s2["x1"][i] - case.pos[None]
        a = np.sort(np.abs(d @ case.frame.T), axis=1)                   # per direction: the frame's three |l|, ascending
        gap = (a[:, 2] - a[:, 1 if tag == "edge" else 0]) / a[:, 2]
        assert gap.size and gap.min() < 1e-7, (k, order, tag, gap)
        tags.add((order, tag))
    assert len(tags) == 6
    assert len(out["direct"]["seen"]["faces"] | out["image"]["seen"]["faces"]) >= 3


@pytest.fixture(scope="module")
def sweep():
    rows = []
    for seed in range(N):
        case = pc.sweep_case(seed)
        out = pc.reference(case)
        rows.append((case, {o: int(r["det"].sum()) for o, r in out.items()}, pc.digest(out)))
    return rows


def test_every_sweep_seed_deposits_something_and_gives_the_pinned_result(sweep):
    for seed, (case, det, dig) in enumerate(sweep):
        assert sum(det.values()) > 0, case.describe()
        assert case.P <= pc.P_MAX and ("image2" not in case.orders or case.K * case.P * case.P <= pc.KPP_MAX), case.describe()
        assert dig == pc.pinned_digests()[f"sweep/{seed}"], case.describe()


def test_the_sweep_covers_the_orders_the_partitions_and_the_options(sweep):
    for order in pc.ORDERS:
        runs = [det[order] for _, det, _ in sweep if order in det]
        assert 3 * len(runs) >= N and 2 * sum(d > 0 for d in runs) >= len(runs), (order, len(runs))
    cases = [c for c, _, _ in sweep]
    assert {c.partition[0] for c in cases} == {"voxel", "octree", "kdtree"}
    for opt in ("image_cull", "image2_prune"):
        assert {getattr(c, opt) for c in cases} == {0, 1}
    assert {c.tables for c in cases} == {"none", "alpha", "alpha+sigma"} and {c.R for c in cases} == {0, 1, 4}
    assert any(c.map and c.K > 256 for c in cases) and any(c.K == 1 for c in cases) and {c.n_weight for c in cases} == {1, 4097, 2 ** 40}
    assert any(np.abs(c.verts[:, :3]).max() > 500 for c in cases) and any(c.verts[:, :3].min() == 0.0 for c in cases)


# ---- the higher orders (tests/test_gpu_path_ambi.py): tests.path_cases.ambi_edge_cases() and ambi_sweep_case(seed)
AMBI = {c.name: c for c in pc.ambi_edge_cases()}
RERUNS = [n for n, c in AMBI.items() if "base" in c.marks]
TWO62 = 2.0 ** 62


def aref(name):
    return pc.reference(AMBI[name], keep=True)


def deposits_of(case, orders=None):
    """Every deposit the reference makes for the case, per path order: rows of (k, bin, m [B], the arrival vector (x, y, z)) -- read where
    tests.ambi_ref.higher_order hands them to tests.ambi_ref.deposit."""
    real, log = ambi_ref.deposit, {}

    def spy(extra, hist, k, bins, v, frac_bits, arrival, counts=None, tallies=None):
        rows.append((int(k), int(bins[0]), magnitude(v, frac_bits)[:, 0], tuple(float(x[0]) for x in arrival())))
        real(extra, hist, k, bins, v, frac_bits, arrival, counts, tallies)
    ambi_ref.deposit = spy
    try:
        for o in orders or case.orders:
            rows = log[o] = []
            pc.reference(case.without(orders=(o,)))
    finally:
        ambi_ref.deposit = real
    return log


def test_the_ambi_file_holds_exactly_the_cases():
    assert set(pc.pinned_ambi_digests()) == {"edge/" + n for n in AMBI} | {f"sweep/{s}" for s in range(AMBI_N)}


@pytest.mark.parametrize("name", list(AMBI))
def test_ambi_edge_case_gives_the_pinned_result_on_c_channels(name):
    case, out = AMBI[name], aref(name)
    assert case.directional and case.order in (2, 3) and case.why
    for res in out.values():
        assert res["hist"].shape == case.shape == (case.K, case.n_bins, case.B, ambi_ref.CHANNELS[case.order])
    assert pc.higher_nonzero(out), case.describe()
    assert pc.digest(out) == pc.pinned_ambi_digests()["edge/" + name], case.describe()


@pytest.mark.parametrize("name", RERUNS)
def test_the_order_changes_nothing_but_the_higher_channels(name):
    """A rerun of a directional edge case: the four channels, det, the counts and what the searches saw are the base case's; the
    case still stands in its oblique room, so the arrivals are oblique; the higher channels of every order it runs hold words."""
    case, out, base = AMBI[name], aref(name), ref(AMBI[name].marks["base"])
    assert EDGES[case.marks["base"]].directional and case.pair == EDGES[case.marks["base"]].pair and set(out) == set(base)
    for o, res in out.items():
        assert (res["hist"][..., :4] == base[o]["hist"]).all() and (res["det"] == base[o]["det"]).all() and res["hist"][..., 4:].any()
        assert res["tallies"] == base[o]["tallies"]
        for key in ("pairs", "cands", "paths"):
            assert res.get(key) == base[o].get(key)
        for key in ("k", "p", "q", "binned", "eligible", "occluded"):
            assert (key in res["seen"]) == (key in base[o]["seen"]) and (key not in res["seen"] or (res["seen"][key] == base[o]["seen"][key]).all())
    if name.startswith("rr-edges"):
        rows = deposits_of(case)
        assert all(min(abs(c) for c in a) > 1e-3 for o in rows for _, _, _, a in rows[o]) and all(rows[o] for o in pc.ORDERS)


def test_the_arrivals_run_along_the_axes_and_the_diagonals():
    """Per path order: an arrival along every axis, a face diagonal in every coordinate plane and a space diagonal, in both signs; the
    components are 0, +-1 and what the division leaves of sqrt(1/2) and sqrt(1/3); with az == 0, Y6 == -0.5 exactly."""
    case = AMBI["arrivals-o3"]
    assert (case.verts == np.round(case.verts * 8) / 8).all() and AMBI["arrivals-o2"].centers.tobytes() == case.centers.tobytes()
    rows = deposits_of(case)
    for o in pc.ORDERS:
        a = np.array([r[3] for r in rows[o]])
        zero, mag = a == 0.0, np.abs(a)
        axial = {(int(np.argmax(m)), float(x[np.argmax(m)])) for x, m, z in zip(a, mag, zero) if z.sum() == 2}
        assert axial >= ({(i, s) for i in range(3) for s in (1.0, -1.0)} if o != "direct" else {(0, 1.0), (0, -1.0), (1, -1.0), (2, -1.0)}), (o, axial)
        face = {(int(np.argmax(z)), tuple(np.sign(x[~z]))) for x, m, z in zip(a, mag, zero) if z.sum() == 1 and len(set(m[~z])) == 1}
        assert {f[0] for f in face} == {0, 1, 2} and len(face) >= 6, (o, face)
        space = [x for x, m, z in zip(a, mag, zero) if z.sum() == 0 and len(set(m)) == 1]
        assert len({tuple(np.sign(x)) for x in space}) >= 2, o
        assert all(abs(abs(x[0]) - np.sqrt(1 / 3)) < 1e-15 for x in space)
        assert all(abs(m[~z][0] - np.sqrt(0.5)) < 1e-15 for m, z in zip(mag, zero) if z.sum() == 1 and len(set(m[~z])) == 1)
        level = a[a[:, 2] == 0.0]
        assert len(level) >= 8 and all(ambi_ref.harmonics(*x)[2] == -0.5 for x in level), o


@pytest.mark.parametrize("fb", (0, 1))
@pytest.mark.parametrize("order", (2, 3))
def test_the_signed_words_meet_ties(order, fb):
    """Receiver 0's direct path: m is 1, 3 and 5 exactly, az == 0, so m * Y6 is -0.5, -1.5 and -2.5, and the word is the tie rounded to
    even: -0, -2, -2.  The words are read back from the reference: nothing else lands in that bin of receiver 0."""
    case = AMBI[f"ties-f{fb}-o{order}"]
    assert case.frac_bits == fb and case.centers.tobytes() == AMBI["arrivals-o3"].centers.tobytes()
    (k, bin_, m, a), = [r for r in deposits_of(case, ("direct",))["direct"] if r[0] == 0]
    y6 = ambi_ref.harmonics(*a)[2]
    assert m.tolist() == [1.0, 3.0, 5.0] and a[2] == 0.0 and y6 == -0.5 and (m * y6).tolist() == [-0.5, -1.5, -2.5]
    words = aref(case.name)["direct"]["hist"][0, bin_]
    assert words[:, 0].tolist() == [1, 3, 5] and words[:, 6].view(np.int64).tolist() == [0, -2, -2]
    assert aref(case.name)["direct"]["tallies"]["ties"] == 0            # m itself is whole: the ties are the signed words' own
    x = m[:, None] * np.array(a)[None, :2]                              # X and Y of the same deposit: m / sqrt(2), no tie, not whole
    assert (words[:, 1:3].view(np.int64) == np.rint(x)).all() and (x != np.rint(x)).all()


@pytest.mark.parametrize("order", (2, 3))
def test_every_signed_channel_stands_at_the_clamp(order):
    case = AMBI[f"clamp-f62-o{order}"]
    rows = deposits_of(case)
    C = ambi_ref.CHANNELS[order]
    hit = np.zeros((2, C), bool)
    n = 0
    for o in pc.ORDERS:
        assert aref(case.name)[o]["tallies"]["saturated"] == 3 * len(rows[o]) > 0          # every add at m == 2^63
        for _, _, m, a in rows[o]:
            w = m[0] * np.array(list(a) + ambi_ref.harmonics(*a, order=order))
            hit[0, 1:] |= w >= TWO62
            hit[1, 1:] |= w <= -TWO62                       # Y6 >= -0.5: it reaches -2^62 and no further
            n += 1
    assert hit[:, 1:].all(), (order, np.argwhere(~hit[:, 1:]))           # every channel 1 .. C - 1, at +2^62 and at -2^62
    h = np.concatenate([aref(case.name)[o]["hist"].reshape(-1, C) for o in pc.ORDERS])
    lone = h[h[:, 0] == np.uint64(1 << 63)]                              # words of a single deposit
    assert len(lone) and ((lone[:, 1:].view(np.int64) == 1 << 62) | (lone[:, 1:].view(np.int64) == -(1 << 62))).any(axis=0).all()


@pytest.mark.parametrize("name", [n for n in AMBI if n.startswith("wide-")])
def test_the_wide_cases_add_128_words_per_deposit(name):
    case, out = AMBI[name], aref(name)
    assert case.B == 8 and case.order == 3 and case.shape[2] * case.shape[3] == 128
    if "second" in name:
        s = out["image2"]["seen"]
        assert case.P == 256 and case.K == 8 and case.orders == ("image2",) and (s["binned"] & ~s["occ"].any(axis=1)).sum() > 50
    else:
        K = int(name.split("-")[1][1:])
        assert case.K == K and case.map == (K > 256) and case.orders == ("direct", "image")
        assert out["image"]["hist"][K - 1, ..., 4:].any() and out["direct"]["hist"][K - 2:, ..., 4:].any()
    for res in out.values():
        assert (res["hist"] != 0).any(axis=(0, 1))[case.power > 0].all() and (case.power > 0).sum() >= 7        # every word of the block, somewhere (one band has no power)


def test_many_paths_of_a_receiver_land_in_one_word():
    case, out = AMBI["one-word-o3"], aref("one-word-o3")
    assert case.n_bins == 1 and case.order == 3
    s1, s2 = out["image"]["seen"], out["image2"]["seen"]
    first = np.bincount(s1["k"][s1["binned"]], minlength=case.K)
    second = np.bincount(s2["k"][s2["binned"]], minlength=case.K)
    assert first.min() >= 50 and second.min() >= 200, (first, second)
    assert (out["image"]["det"][:, 0] == first).all() and (out["image2"]["det"][:, 0] == second).all() and not out["image2"]["det"][:, 1].any()
    signed = ambi_ref.signed(out["image2"]["hist"])
    assert (signed < 0).any() and (signed > 0).any()                     # sums of both signs: words that wrap as uint64


@pytest.mark.parametrize("kind", ("voxel", "octree", "kdtree"))
def test_order_3_runs_under_every_partition_with_occluders(kind):
    case, out = AMBI[f"{kind}-o3"], aref(f"{kind}-o3")
    assert case.partition[0] == kind and case.order == 3 and case.P > 48 and set(out) == set(pc.ORDERS)
    normals = pc.oracle_of(case)[2]
    assert (np.abs(normals[:48]) > 1e-3).all()                           # an oblique room
    assert out["image"]["seen"]["occ_rcv"].any() or out["image"]["seen"]["occ_src"].any() or out["image2"]["seen"]["occ"].any()
    assert all(res["det"][:, 0].sum() > 0 and res["hist"][..., 4:].any() for res in out.values())


@pytest.fixture(scope="module")
def ambi_sweep():
    rows = []
    for seed in range(AMBI_N):
        case = pc.ambi_sweep_case(seed)
        out = pc.reference(case)
        rows.append((case, sum(int(r["det"].sum()) for r in out.values()), pc.digest(out), pc.higher_nonzero(out)))
    return rows


def test_every_ambi_sweep_seed_is_its_base_seed_widened_and_gives_the_pinned_result(ambi_sweep):
    for seed, (case, det, dig, higher) in enumerate(ambi_sweep):
        base = pc.sweep_case(seed)
        assert case.directional and case.order in (2, 3) and det > 0, case.describe()
        assert int(np.prod(case.shape)) <= pc.WORDS_MAX and case.K * case.B * case.shape[3] <= max(pc.AMBI_KBC_MAX, case.B * case.shape[3])
        assert case.n_bins * case.bin_len >= base.n_bins * base.bin_len and case.centers.tobytes() == base.centers[:case.K].tobytes()
        for f in ("partition", "frac_bits", "n_weight", "orders", "image_cull", "image2_prune", "R", "map"):
            assert getattr(case, f) == getattr(base, f), (seed, f)
        assert case.verts.tobytes() == base.verts.tobytes() and case.pos.tobytes() == base.pos.tobytes() and case.power.tobytes() == base.power.tobytes()
        assert dict(digest=dig, higher=higher) == pc.pinned_ambi_digests()[f"sweep/{seed}"], case.describe()


def test_the_ambi_sweep_is_not_vacuous_in_the_higher_channels(ambi_sweep):
    """At most 10 of 100 seeds leave the channels 4 .. C - 1 all zero (nothing binned, or a low frac_bits that rounds every m * Y to 0)."""
    zero = [seed for seed, row in enumerate(ambi_sweep) if not row[3]]
    assert 10 * len(zero) <= AMBI_N, zero
    assert {row[0].order for row in ambi_sweep} == {2, 3}
    for order in pc.ORDERS:
        assert sum(1 for row in ambi_sweep if order in row[0].orders and row[3]) >= AMBI_N // 4, order
