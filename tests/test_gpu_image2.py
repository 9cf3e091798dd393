"""Second-order image sources on the MI355X (include/hare_hip.h, "receivers", "Image sources (second order)").  hare_image2_device against
tests/image2_ref.py, byte for byte on the histogram and the detections, over image2_ref.cases() -- the four scenes of
tests/test_gpu_image.py (P = 12, 54, 56, 972), the three partitions, K = 1, 8, 256 linear and 257 as a map, with and without channels --
accumulating onto words that are not zero, with guard bytes behind the work array untouched and lists of exactly the counts found; a list
one short (nothing added, both counts reported, HARE_E_NOMEM from the host call); "image2_prune" 0 against 1 (equal bytes, equal path
count, every reference path's (p, q) in the pruned list).  The identity

    hist(IMAGE | IMAGE2, bounces) = hist(0, bounces) - hist(0, 3) + hist(0, 1) + image + image2        (wrapping uint64; detections alike)

on hare_receive_source without a scattering table, with and without HARE_RECEIVE_DIRECT; a scattering scene with and without rain against
the reference's per-ray suppression at 1 / 2 / 3 / 5 casts; the sharded, the reduced and the device call; the flag refused alone; and a call
without the flag against the bytes it returns when the work array ends where it ended before the flag existed."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests import image2_ref as i2
from tests import image_ref as ir
from tests import source_ref as sr
from tests.test_gpu_image import (B3, FRAC, PART, R3, SCENE, SRC, device_u64, image_term, library_partition, scene_for, scene_of, tables)

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def run_device(torch, g, case, max_cands, max_paths, P):
    """hare_image2_device of the case onto random words: (added histogram, added detections, candidates found, paths found, the candidate
    list's (p, q) rows)."""
    K, words = case.K, int(np.prod(case.shape))
    rng = np.random.default_rng(3)
    base_h = rng.integers(0, 2 ** 64, words + GUARD, dtype=np.uint64)
    base_d = rng.integers(0, 2 ** 64, 2 * K + GUARD, dtype=np.uint64)
    d_hist, d_det = device_u64(torch, base_h), device_u64(torch, base_d)
    wb = H.Voxel_Grid.image2_work_bytes(P, max_cands, max_paths)
    d_work = torch.full((wb + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g.Image2_device(case.n_weight, case.n_bins, case.bin_len, case.frac_bits, max_cands, max_paths, d_work.data_ptr(), d_hist.data_ptr(),
                    d_det.data_ptr(), directional=case.directional)
    torch.cuda.synchronize()
    hist, det, work = d_hist.cpu().numpy().view(np.uint64), d_det.cpu().numpy().view(np.uint64), d_work.cpu().numpy()
    assert (work[wb:] == FILL).all() and (hist[words:] == base_h[words:]).all() and (det[2 * K:] == base_d[2 * K:]).all()
    nc, m = (int(x) for x in work[:16].view(np.uint64))
    pq = work[256 + 32 * P + 24 * max_cands:][:8 * max_cands].view(np.int32).reshape(max_cands, 2)          # behind the images and S''
    with np.errstate(over="ignore"):
        return ((hist[:words] - base_h[:words]).reshape(case.shape), (det[:2 * K] - base_d[:2 * K]).reshape(K, 2), nc, m,
                pq[:min(nc, max_cands)].copy())


def case_named(name):
    return next(c for c in i2.cases() if c.name == name)


@pytest.mark.parametrize("case", i2.cases(), ids=lambda c: c.name)
def test_image2_device_matches_the_reference(torch, case):
    want = i2.reference(case)
    g, T = scene_of(case)
    g.set_option("image2_prune", 0)                                   # every ordered pair with a second image: the reference's own candidate set
    got_h, got_d, nc, m, pq = run_device(torch, g, case, max(1, want["cands"]), max(1, want["paths"]), T.Polygon_Count)      # lists of exactly the counts
    print(case.name, "cands", want["cands"], "paths", want["paths"], "free", int(want["det"].sum()))
    c = want["seen"]["cands"]
    assert (nc, m) == (want["cands"], want["paths"])
    assert sorted(map(tuple, pq.tolist())) == sorted(zip(c["p"].tolist(), c["q"].tolist()))
    bad = np.argwhere(got_d != want["det"])
    assert bad.size == 0, (bad[:4], got_d[tuple(bad[0])], want["det"][tuple(bad[0])])
    bad = np.argwhere(got_h != want["hist"])
    assert bad.size == 0, (len(bad), bad[:4], got_h[tuple(bad[0])], want["hist"][tuple(bad[0])])


@pytest.mark.parametrize("name", ("box12-K8-dir", "quads-map257-dir", "baffle-K8", "box972-K8-dir"))
def test_the_prune_changes_nothing_and_keeps_every_reference_path(torch, name):
    case = case_named(name)
    want = i2.reference(case)
    g, T = scene_of(case)
    out = {}
    for prune in (1, 0):
        g.set_option("image2_prune", prune)
        out[prune] = run_device(torch, g, case, want["cands"] + 5, want["paths"] + 5, T.Polygon_Count)
    print(name, "candidates pruned", out[1][2], "of", out[0][2], "paths", out[1][3])
    assert (out[0][0] == out[1][0]).all() and (out[0][1] == out[1][1]).all() and out[0][3] == out[1][3] == want["paths"]
    assert out[0][2] == want["cands"] and out[1][2] <= out[0][2]
    if name == "box972-K8-dir":                                       # small polygons, narrow pyramids: the filter must bite, not merely do no harm
        assert out[1][2] * 4 < out[0][2], (out[1][2], out[0][2])
    kept = set(map(tuple, out[1][4].tolist()))
    s = want["seen"]
    assert set(zip(s["p"].tolist(), s["q"].tolist())) <= kept       # no reference path's pair is missing from the pruned list
    assert (out[1][0] == want["hist"]).all() and (out[1][1] == want["det"]).all()


@pytest.mark.parametrize("short", ("cands", "paths"))
def test_a_list_one_short_adds_nothing_and_reports_the_counts(torch, short):
    case = case_named("baffle-K8")
    want = i2.reference(case)
    g, T = scene_of(case)
    g.set_option("image2_prune", 0)
    nc, m = want["cands"] - (short == "cands"), want["paths"] - (short == "paths")
    got_h, got_d, fc, fm, _ = run_device(torch, g, case, nc, m, T.Polygon_Count)
    assert fc == want["cands"] and (fm == want["paths"] or short == "cands") and not got_h.any() and not got_d.any()
    g.set_option("image2_max_cands", nc).set_option("image2_max_paths", m)
    with pytest.raises(H.HareError) as e:
        g.Receive_source(65, 3, case.n_bins, case.bin_len, image=True, image2=True)
    assert e.value.code == capi.HARE_E_NOMEM and str(want["cands"]) in str(e.value)
    if short == "paths":
        assert str(want["paths"]) in str(e.value)
    g.set_option("image2_max_cands", want["cands"]).set_option("image2_max_paths", want["paths"])
    assert g.Receive_source(65, 3, case.n_bins, case.bin_len, image=True, image2=True)[2].sum() > 0


def test_a_scene_without_a_candidate_deposits_nothing_through_the_host_call_too():
    """corner3: both counts come back 0 -- the path stage leaves in its first block, the deposit finds nothing -- and the host call's
    results are those of the call with the first-order flag alone."""
    case = case_named("corner3-K8-nocands")
    g, T = scene_of(case)
    both = g.Receive_source(4097, 3, case.n_bins, case.bin_len, image=True, image2=True)
    first = g.Receive_source(4097, 3, case.n_bins, case.bin_len, image=True)
    assert i2.reference(case)["cands"] == 0
    # cast 2 is still suppressed for the twice-specular rays, so compare the deposits' part: one cast, where nothing is suppressed
    one2 = g.Receive_source(4097, 1, case.n_bins, case.bin_len, image=True, image2=True)
    one1 = g.Receive_source(4097, 1, case.n_bins, case.bin_len, image=True)
    assert (one2[0] == one1[0]).all() and (one2[2] == one1[2]).all() and one2[3].tobytes() == one1[3].tobytes()
    assert both[3].tobytes() == first[3].tobytes() and both[4] == first[4]


# ---- the identity on hare_receive_source (no scattering table)
def image2_term(centers, radii, n, n_bins, bin_len, directional, partition=PART, scatter=False):
    verts, nverts, _ = ir.mesh_of(SCENE)
    _, o, normals = ir.oracle_of(SCENE, partition)
    alpha, sigma = tables()
    K = centers.shape[0]
    hist = np.zeros((K, n_bins, B3, 4) if directional else (K, n_bins, B3), np.uint64)
    det = np.zeros((K, 2), np.uint64)
    i2.image2(o, verts, nverts, normals, SRC, sr.powers(B3), sr.rotation(), R3, sr.table(R3, B3), alpha, sigma if scatter else None, centers, radii,
              n, n_bins, bin_len, FRAC, hist, det)
    return hist, det


@pytest.mark.parametrize("direct", (False, True), ids=("image2", "direct+image2"))
@pytest.mark.parametrize("mode", ("plain", "directional", "map"))
def test_the_flags_replace_the_specular_part_of_casts_1_and_2_by_the_deposits(mode, direct):
    g, centers, radii, kw, n_bins, bin_len = scene_for(mode)
    n = 4097
    i_hist, i_det = image_term(centers, radii, n, n_bins, bin_len, kw["directional"])
    j_hist, j_det = image2_term(centers, radii, n, n_bins, bin_len, kw["directional"])
    assert int(j_det.sum()) > 0
    call = lambda bounces, flag: g.Receive_source(n, bounces, n_bins, bin_len, frac_bits=FRAC, direct=direct, image=flag, image2=flag, **kw)
    one, three = call(1, False), call(3, False)
    for bounces in (1, 2, 3, 5):
        plain = one if bounces == 1 else (three if bounces == 3 else call(bounces, False))
        flag = call(bounces, True)
        with np.errstate(over="ignore"):
            if bounces >= 3:
                want_h, want_d = plain[0] - three[0] + one[0] + i_hist + j_hist, plain[2] - three[2] + one[2] + i_det + j_det
            else:                                                          # nothing more is suppressed than the first-order flag suppresses
                first = g.Receive_source(n, bounces, n_bins, bin_len, frac_bits=FRAC, direct=direct, image=True, **kw)
                want_h, want_d = first[0] + j_hist, first[2] + j_det
        assert (flag[0] == want_h).all(), (mode, direct, bounces, np.argwhere(flag[0] != want_h)[:4])
        assert (flag[2] == want_d).all(), (mode, direct, bounces)
        assert flag[3].tobytes() == plain[3].tobytes() and flag[4] == plain[4], (mode, direct, bounces)
    with np.errstate(over="ignore"):
        assert (three[2] - call(2, False)[2]).any()                      # cast 2 does detect without the flag


# ---- a scattering table: per-ray suppression, against the reference
@pytest.mark.parametrize("rain", (False, True), ids=("scatter", "rain"))
def test_with_a_scattering_table_the_twice_specular_rays_of_cast_2_are_suppressed(rain):
    g, centers, radii, kw, n_bins, bin_len = scene_for("plain", scatter=True)
    To, o, _ = ir.oracle_of(SCENE, PART)
    alpha, sigma = tables()
    n = 4097
    rays, state = sr.emit(21, 0, n, np.array(SRC), sr.powers(B3), sr.rotation(), R3, sr.table(R3, B3))
    i_hist, i_det = image_term(centers, radii, n, n_bins, bin_len, False, scatter=True)
    j_hist, j_det = image2_term(centers, radii, n, n_bins, bin_len, False, scatter=True)
    for bounces in (1, 2, 3, 5):
        h, d, st, split = i2.suppressed2(To, o, rays, state, bounces, centers, radii, n_bins, bin_len, FRAC, alpha=alpha, sigma=sigma, seed=5, rain=rain)
        got = g.Receive_source(n, bounces, n_bins, bin_len, frac_bits=FRAC, image=True, image2=True, rain=rain)
        plain = g.Receive_source(n, bounces, n_bins, bin_len, frac_bits=FRAC, rain=rain)
        with np.errstate(over="ignore"):
            assert (got[0] == h + i_hist + j_hist).all(), (rain, bounces, np.argwhere(got[0] != h + i_hist + j_hist)[:4])
            assert (got[2] == d + i_det + j_det).all(), (rain, bounces)
        assert got[3].tobytes() == st.tobytes() == plain[3].tobytes() and got[4] == plain[4]
        if bounces > 2:
            assert split["twice"] > 300 and split["other"] > 300


# ---- the other calls
N_OTHER, CASTS_OTHER = 4097, 4


def test_sharded_over_two_scenes_deposits_once():
    a, centers, radii, kw, n_bins, bin_len = scene_for("plain", scatter=True)
    b = scene_for("plain", scatter=True)[0]
    for n in (N_OTHER, 1):
        one = a.Receive_source(n, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, image=True, image2=True, direct=True)
        two = H.Spatial_Partition.Receive_source_sharded([a, b], n, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, image=True, image2=True, direct=True)
        assert (one[0] == two[0]).all() and (one[2] == two[2]).all() and one[3].tobytes() == two[3].tobytes() and one[4] == two[4], n
        first = a.Receive_source(n, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, image=True, direct=True)
        assert (one[0] != first[0]).any()


def test_reduced_with_the_flag_is_the_reduction_of_the_flagged_histogram():
    g, centers, radii, kw, n_bins, bin_len = scene_for("map")
    spec = dict(windows=[(0, n_bins), (0, 8), (8, n_bins)], levels=H.decay_levels([-5, -10]).tolist())
    hist, _, det, state, ctr = g.Receive_source(N_OTHER, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, image=True, image2=True)
    sums, cross, det2, state2, ctr2 = g.Receive_source_reduced(N_OTHER, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, image=True, image2=True, **spec)
    want_sums, want_cross = g.hist_reduce(hist, **spec)
    assert (sums == want_sums).all() and (cross == want_cross).all() and (det == det2).all() and state.tobytes() == state2.tobytes() and ctr == ctr2
    first = g.Receive_source_reduced(N_OTHER, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, image=True, **spec)
    assert (first[0] != sums).any()                                              # the flag is seen


def device_loop(torch, g, n, K, n_bins, bin_len, image, image2, work_bytes, rain=False):
    d_rays = torch.empty(n * 6, dtype=torch.float64, device="cuda")
    d_state = torch.empty(n * (1 + B3), dtype=torch.float64, device="cuda")
    d_work = torch.full((work_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    d_last = torch.zeros(n * 56, dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros(K * n_bins * B3, dtype=torch.int64, device="cuda")
    d_det = torch.zeros(2 * K, dtype=torch.int64, device="cuda")
    g.emit_device(n, d_rays.data_ptr(), d_state.data_ptr())
    if image2:
        P, C, M = ir.mesh_of(SCENE)[0].shape[0], 4096, 32768
        d_i1 = torch.zeros(H.Voxel_Grid.image_work_bytes(K, P, M), dtype=torch.uint8, device="cuda")
        d_i2 = torch.zeros(H.Voxel_Grid.image2_work_bytes(P, C, M), dtype=torch.uint8, device="cuda")
        g.Image_device(n, n_bins, bin_len, FRAC, M, d_i1.data_ptr(), d_hist.data_ptr(), d_det.data_ptr())
        g.Image2_device(n, n_bins, bin_len, FRAC, C, M, d_i2.data_ptr(), d_hist.data_ptr(), d_det.data_ptr())
    g.receive_device(n, d_rays.data_ptr(), CASTS_OTHER, n_bins, bin_len, FRAC, d_state.data_ptr(), d_work.data_ptr(), d_last.data_ptr(),
                     d_hist.data_ptr(), d_det.data_ptr(), image=image, image2=image2, rain=rain)
    torch.cuda.synchronize()
    work = d_work.cpu().numpy()
    assert (work[work_bytes:] == FILL).all()                                     # nothing behind the work array the call was promised
    return dict(hist=d_hist.cpu().numpy().view(np.uint64).reshape(K, n_bins, B3), det=d_det.cpu().numpy().view(np.uint64).reshape(K, 2),
                state=d_state.cpu().numpy().reshape(1 + B3, n), rays=d_rays.cpu().numpy(), last=d_last.cpu().numpy(), work=work)


@pytest.mark.parametrize("as_map", (False, True), ids=("linear", "map"))
def test_receive_device_with_the_flags_and_the_two_deposits_reproduce_receive_source(torch, as_map):
    g, centers, radii, kw, n_bins, bin_len = scene_for("map" if as_map else "plain", ir.PARTITIONS[2], scatter=True)
    n, K = N_OTHER, centers.shape[0]
    want = g.Receive_source(n, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, image=True, image2=True)
    got = device_loop(torch, g, n, K, n_bins, bin_len, True, True, H.Voxel_Grid.receive_work_bytes(n, image2=True))
    off = device_loop(torch, g, n, K, n_bins, bin_len, False, False, H.Voxel_Grid.receive_work_bytes(n))
    assert (got["hist"] == want[0]).all() and (got["det"] == want[2]).all() and got["state"].tobytes() == want[3].tobytes()
    for what in ("rays", "state", "last"):                                       # the flags change deposits only
        assert got[what].tobytes() == off[what].tobytes(), what
    assert (got["hist"] != off["hist"]).any()
    assert set(np.unique(got["work"][8 * n:9 * n]).tolist()) <= {0, 1, FILL}     # the byte per ray, behind the loop's 2 n int32


@pytest.mark.parametrize("rain", (False, True), ids=("plain", "rain"))
def test_a_call_without_the_flag_touches_the_bytes_it_touched_before(torch, rain):
    """The regression guard: without HARE_RECEIVE_IMAGE2 the work array ends where it ended before the flag existed -- the guard bytes
    behind 8 n (HARE_RECEIVE_RAIN_WORK_BYTES(n) with rain) stay untouched (device_loop asserts it) -- and the results are those of the host
    call, with HARE_RECEIVE_IMAGE as without it."""
    g, centers, radii, kw, n_bins, bin_len = scene_for("plain", scatter=True)
    n, K = N_OTHER, centers.shape[0]
    for image in (False, True):
        got = device_loop(torch, g, n, K, n_bins, bin_len, image, False, H.Voxel_Grid.receive_work_bytes(n, rain=rain), rain=rain)
        want = g.Receive_source(n, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, image=image, rain=rain)
        if image:                                                                # the device call suppresses only: add the deposit's term
            i_hist, i_det = image_term(centers, radii, n, n_bins, bin_len, False, scatter=True)
            with np.errstate(over="ignore"):
                got["hist"], got["det"] = got["hist"] + i_hist, got["det"] + i_det
        assert (got["hist"] == want[0]).all() and (got["det"] == want[2]).all() and got["state"].tobytes() == want[3].tobytes(), image


def test_the_flag_is_refused_without_the_first_order_flag():
    g, centers, radii, kw, n_bins, bin_len = scene_for("plain")
    for call in (lambda: g.Receive_source(65, 3, n_bins, bin_len, image2=True),
                 lambda: g.Receive_source(65, 3, n_bins, bin_len, image2=True, direct=True),
                 lambda: g.Receive_source_reduced(65, 3, n_bins, bin_len, windows=[(0, n_bins)], image2=True),
                 lambda: H.Spatial_Partition.Receive_source_sharded([g], 65, 3, n_bins, bin_len, image2=True),
                 lambda: g.receive_device(8, 1 << 20, 3, n_bins, bin_len, 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20, image2=True)):
        with pytest.raises(H.HareError) as e:
            call()
        assert e.value.code == capi.HARE_E_INVALID and "HARE_RECEIVE_IMAGE2" in str(e.value)
    assert g.Receive_source(65, 3, n_bins, bin_len, image=True, image2=True)[2].sum() > 0
