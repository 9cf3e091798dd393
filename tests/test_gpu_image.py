"""First-order image sources on the MI355X (include/hare_hip.h, "receivers", "Image sources (first order)").  hare_image_device against
tests/image_ref.py, byte for byte on the histogram and the detections, over image_ref.cases() -- four scenes (the 12- and the 972-triangle
shoebox, a box of quadrilaterals, a box with a baffle), the three partitions, K = 1 .. 256 linear and 257 as a map, B = 1, 3, 8, with and
without a directivity table, absorption alone and with scattering, frac_bits 0, 40, 62, one bin and many, one and four channels, n_weight
1, 4 097, 2^40 -- accumulating onto a histogram that is not zero, with guard words behind every buffer untouched, the three HIP call
counters unmoved and a pair list of exactly the pairs found; the list one pair short (nothing added, the count reported, HARE_E_NOMEM from
the host call); "image_cull" 0 against 1 (equal bytes, equal pair lists as sets).  The identity

    hist(flag, bounces) = hist(no flag, bounces) - hist(no flag, 2) + hist(no flag, 1) + image           (wrapping uint64; detections alike)

on hare_receive_source without a scattering table in the modes of tests/test_gpu_direct.py, with and without HARE_RECEIVE_DIRECT; a
scattering scene with and without rain against the reference's per-ray suppression; the sharded, the reduced and the device call."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests import image_ref as ir
from tests import source_ref as sr
from tests.receive_harness import CALL_COUNTERS

pytestmark = pytest.mark.gpu

GUARD = 64                                   # bytes behind d_work; 8-byte words behind d_hist and d_detections
FILL = 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def library_partition(partition, scene):
    verts, nverts, _ = ir.mesh_of(scene)
    T = H.Topology(verts, nverts)
    kind, *par = partition
    return H.Voxel_Grid([T], par[0]) if kind == "voxel" else (H.Octree if kind == "octree" else H.KDTree)([T], *par), T


def device_u64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1)).to("cuda")


def scene_of(case):
    g, T = library_partition(case.partition, case.scene)
    centers, radii = case.receivers()
    (g.set_receiver_map if case.map else g.set_receivers)(centers, radii)
    alpha, sigma = case.absorption()
    if alpha is not None:
        g.set_absorption(alpha)
    if sigma is not None:
        g.set_scattering(sigma)
    pos, power, frame, R, gain = case.source()
    g.set_source(pos, power=power, frame=frame, gain=gain)
    return g, T


def run_device(torch, g, case, max_pairs, P):
    """hare_image_device of the case onto random words: (added histogram, added detections, pairs found, the list's (k, p) rows)."""
    K, words = case.K, int(np.prod(case.shape))
    rng = np.random.default_rng(3)
    base_h = rng.integers(0, 2 ** 64, words + GUARD, dtype=np.uint64)           # the call ACCUMULATES: onto words that are not zero
    base_d = rng.integers(0, 2 ** 64, 2 * K + GUARD, dtype=np.uint64)
    d_hist, d_det = device_u64(torch, base_h), device_u64(torch, base_d)
    wb = H.Voxel_Grid.image_work_bytes(K, P, max_pairs)
    d_work = torch.full((wb + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = [g.get_option(o) for o in CALL_COUNTERS]
    g.Image_device(case.n_weight, case.n_bins, case.bin_len, case.frac_bits, max_pairs, d_work.data_ptr(), d_hist.data_ptr(), d_det.data_ptr(),
                   directional=case.directional)
    after = [g.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    assert after == before, dict(zip(CALL_COUNTERS, (a - b for a, b in zip(after, before))))
    hist, det, work = d_hist.cpu().numpy().view(np.uint64), d_det.cpu().numpy().view(np.uint64), d_work.cpu().numpy()
    assert (work[wb:] == FILL).all() and (hist[words:] == base_h[words:]).all() and (det[2 * K:] == base_d[2 * K:]).all()
    found = int(work[:8].view(np.uint64)[0])
    kp = work[256 + 32 * P + 112 * max_pairs:][:8 * max_pairs].view(np.int32).reshape(max_pairs, 2)      # behind the shadow rays and their t_max
    with np.errstate(over="ignore"):
        return ((hist[:words] - base_h[:words]).reshape(case.shape), (det[:2 * K] - base_d[:2 * K]).reshape(K, 2), found,
                kp[:min(found, max_pairs)].copy())


# ---- hare_image_device against the reference
@pytest.mark.parametrize("case", ir.cases(), ids=lambda c: c.name)
def test_image_device_matches_the_reference(torch, case):
    want = ir.reference(case)
    g, T = scene_of(case)
    got_h, got_d, found, kp = run_device(torch, g, case, max(1, want["pairs"]), T.Polygon_Count)      # a list of exactly the pairs there are
    s = want["seen"]
    print(case.name, "pairs", want["pairs"], "free", int(want["det"].sum()), "words", int((want["hist"] != 0).sum()))
    assert found == want["pairs"]
    assert sorted(map(tuple, kp.tolist())) == sorted(zip(s["k"].tolist(), s["p"].tolist()))          # the list, as a set
    bad = np.argwhere(got_d != want["det"])
    assert bad.size == 0, (bad[:4], got_d[tuple(bad[0])], want["det"][tuple(bad[0])])
    bad = np.argwhere(got_h != want["hist"])
    assert bad.size == 0, (len(bad), bad[:4], got_h[tuple(bad[0])], want["hist"][tuple(bad[0])])


def case_named(name):
    return next(c for c in ir.cases() if c.name == name)


def test_a_list_one_pair_short_adds_nothing_and_reports_the_count(torch):
    case = case_named("baffle-K64")
    want = ir.reference(case)
    g, T = scene_of(case)
    got_h, got_d, found, _ = run_device(torch, g, case, want["pairs"] - 1, T.Polygon_Count)
    assert found == want["pairs"] and not got_h.any() and not got_d.any()
    g.set_option("image_max_pairs", want["pairs"] - 1)
    with pytest.raises(H.HareError) as e:
        g.Receive_source(65, 2, case.n_bins, case.bin_len, image=True)
    assert e.value.code == capi.HARE_E_NOMEM and str(want["pairs"]) in str(e.value)
    g.set_option("image_max_pairs", want["pairs"])
    assert g.Receive_source(65, 2, case.n_bins, case.bin_len, image=True)[2].sum() > 0


@pytest.mark.parametrize("name", ("box972-K65-dir", "quads-map257-dir", "baffle-K64"))
def test_the_pre_cull_changes_nothing(torch, name):
    case = case_named(name)
    want = ir.reference(case)
    g, T = scene_of(case)
    out = {}
    for cull in (1, 0):
        g.set_option("image_cull", cull)
        out[cull] = run_device(torch, g, case, want["pairs"] + 5, T.Polygon_Count)
    assert (out[0][0] == out[1][0]).all() and (out[0][1] == out[1][1]).all() and out[0][2] == out[1][2] == want["pairs"]
    assert sorted(map(tuple, out[0][3].tolist())) == sorted(map(tuple, out[1][3].tolist()))
    assert (out[1][0] == want["hist"]).all()


# ---- the identity on hare_receive_source (no scattering table)
B3, R3, FRAC = 3, 4, 30
SCENE, PART, SRC = "baffle", ir.PARTITIONS[0], (2.0, 1.0, 1.0)
MODES = ("plain", "directional", "time_limit", "floor", "map")
SIZES, CASTS = (65, 4097), (1, 2, 5)


def receivers_of(as_map):
    return ir.ImageCase("identity", SCENE, PART, 300 if as_map else 6, as_map, B3, R3, "alpha", FRAC, 64, 0.25, False, 1, pos=SRC).receivers()


def tables():
    P = ir.mesh_of(SCENE)[0].shape[0]
    rng = np.random.default_rng(9)
    return rng.uniform(0.05, 0.5, (P, B3)), rng.uniform(0.05, 0.6, (P, B3))


def scene_for(mode, partition=PART, scatter=False):
    g, T = library_partition(partition, SCENE)
    centers, radii = receivers_of(mode == "map")
    (g.set_receiver_map if mode == "map" else g.set_receivers)(centers, radii)
    alpha, sigma = tables()
    g.set_absorption(alpha)
    if scatter:
        g.set_scattering(sigma).set_option("scatter_seed", 5)
    if mode == "floor":
        g.set_option("receive_floor_bits", 2).set_option("receive_roulette", 1)
    g.set_source(SRC, power=sr.powers(B3), frame=sr.rotation(), gain=sr.table(R3, B3)).set_option("source_seed", 21)
    kw = dict(directional=mode == "directional", time_limit=mode == "time_limit")
    n_bins, bin_len = (24, 0.25) if mode == "time_limit" else (64, 0.25)         # the time limit bites: 6 m of histogram
    return g, centers, radii, kw, n_bins, bin_len


def image_term(centers, radii, n, n_bins, bin_len, directional, partition=PART, scatter=False):
    verts, nverts, _ = ir.mesh_of(SCENE)
    _, o, normals = ir.oracle_of(SCENE, partition)
    alpha, sigma = tables()
    K = centers.shape[0]
    hist = np.zeros((K, n_bins, B3, 4) if directional else (K, n_bins, B3), np.uint64)
    det = np.zeros((K, 2), np.uint64)
    ir.image(o, verts, nverts, normals, SRC, sr.powers(B3), sr.rotation(), R3, sr.table(R3, B3), alpha, sigma if scatter else None, centers, radii, n,
             n_bins, bin_len, FRAC, hist, det)
    return hist, det


@pytest.mark.parametrize("direct", (False, True), ids=("image", "direct+image"))
@pytest.mark.parametrize("mode", MODES)
def test_the_flag_replaces_the_specular_part_of_cast_1_by_the_deposit(mode, direct):
    g, centers, radii, kw, n_bins, bin_len = scene_for(mode)
    deposits = 0
    for n in SIZES:
        i_hist, i_det = image_term(centers, radii, n, n_bins, bin_len, kw["directional"])
        deposits += int(i_det.sum())
        call = lambda bounces, image: g.Receive_source(n, bounces, n_bins, bin_len, frac_bits=FRAC, direct=direct, image=image, **kw)
        one, two = call(1, False), call(2, False)
        for bounces in CASTS:
            plain = one if bounces == 1 else (two if bounces == 2 else call(bounces, False))
            flag = call(bounces, True)
            tag = (mode, direct, n, bounces)
            with np.errstate(over="ignore"):
                want_h = plain[0] + i_hist if bounces == 1 else plain[0] - two[0] + one[0] + i_hist
                want_d = plain[2] + i_det if bounces == 1 else plain[2] - two[2] + one[2] + i_det
            assert (flag[0] == want_h).all(), (tag, np.argwhere(flag[0] != want_h)[:4])
            assert (flag[2] == want_d).all(), tag
            assert flag[3].tobytes() == plain[3].tobytes() and flag[4] == plain[4], tag          # state and counters
    with np.errstate(over="ignore"):
        assert deposits > 0 and (two[2] - one[2]).any()                  # something was deposited, and cast 1 does detect without the flag


# ---- a scattering table: per-ray suppression, against the reference
@pytest.mark.parametrize("rain", (False, True), ids=("scatter", "rain"))
def test_with_a_scattering_table_the_specular_rays_of_cast_1_are_suppressed(rain):
    g, centers, radii, kw, n_bins, bin_len = scene_for("plain", scatter=True)
    To, o, _ = ir.oracle_of(SCENE, PART)
    alpha, sigma = tables()
    n = 4097
    rays, state = sr.emit(21, 0, n, np.array(SRC), sr.powers(B3), sr.rotation(), R3, sr.table(R3, B3))
    i_hist, i_det = image_term(centers, radii, n, n_bins, bin_len, False, scatter=True)
    for bounces in CASTS:
        h, d, st, split = ir.suppressed(To, o, rays, state, bounces, centers, radii, n_bins, bin_len, FRAC, alpha=alpha, sigma=sigma, seed=5, rain=rain)
        got = g.Receive_source(n, bounces, n_bins, bin_len, frac_bits=FRAC, image=True, rain=rain)
        plain = g.Receive_source(n, bounces, n_bins, bin_len, frac_bits=FRAC, rain=rain)
        with np.errstate(over="ignore"):
            assert (got[0] == h + i_hist).all(), (rain, bounces, np.argwhere(got[0] != h + i_hist)[:4])
            assert (got[2] == d + i_det).all(), (rain, bounces)
        assert got[3].tobytes() == st.tobytes() == plain[3].tobytes() and got[4] == plain[4]
        if bounces > 1:
            assert split["specular"] > 500 and split["diffuse"] > 500


# ---- the other calls
N_OTHER, CASTS_OTHER = 4097, 3


def test_sharded_over_two_scenes_deposits_once():
    a, centers, radii, kw, n_bins, bin_len = scene_for("plain", scatter=True)
    b = scene_for("plain", scatter=True)[0]
    for n in (N_OTHER, 1):                                                       # n = 1: scenes[0]'s shard is empty, scenes[1] deposits
        one = a.Receive_source(n, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, image=True, direct=True)
        two = H.Spatial_Partition.Receive_source_sharded([a, b], n, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, image=True, direct=True)
        assert (one[0] == two[0]).all() and (one[2] == two[2]).all() and one[3].tobytes() == two[3].tobytes() and one[4] == two[4], n
        assert one[2].sum() > 0


def test_reduced_with_the_flag_is_the_reduction_of_the_flagged_histogram():
    g, centers, radii, kw, n_bins, bin_len = scene_for("map")
    spec = dict(windows=[(0, n_bins), (0, 8), (8, n_bins)], levels=H.decay_levels([-5, -10]).tolist())
    hist, _, det, state, ctr = g.Receive_source(N_OTHER, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, image=True)
    sums, cross, det2, state2, ctr2 = g.Receive_source_reduced(N_OTHER, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, image=True, **spec)
    want_sums, want_cross = g.hist_reduce(hist, **spec)
    assert (sums == want_sums).all() and (cross == want_cross).all() and (det == det2).all() and state.tobytes() == state2.tobytes() and ctr == ctr2
    plain = g.Receive_source_reduced(N_OTHER, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, **spec)
    assert (plain[0] != sums).any()                                              # the flag is seen


@pytest.mark.parametrize("as_map", (False, True), ids=("linear", "map"))
def test_receive_device_with_the_flag_and_image_device_reproduce_receive_source(torch, as_map):
    g, centers, radii, kw, n_bins, bin_len = scene_for("map" if as_map else "plain", ir.PARTITIONS[2], scatter=True)
    n, K, P, M = N_OTHER, centers.shape[0], ir.mesh_of(SCENE)[0].shape[0], 4096
    want = g.Receive_source(n, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, image=True)
    out = {}
    for image in (True, False):
        d_rays = torch.empty(n * 6, dtype=torch.float64, device="cuda")
        d_state = torch.empty(n * (1 + B3), dtype=torch.float64, device="cuda")
        d_work = torch.zeros(H.Voxel_Grid.receive_work_bytes(n), dtype=torch.uint8, device="cuda")
        d_iwork = torch.zeros(H.Voxel_Grid.image_work_bytes(K, P, M), dtype=torch.uint8, device="cuda")
        d_last = torch.zeros(n * 56, dtype=torch.uint8, device="cuda")
        d_hist = torch.zeros(K * n_bins * B3, dtype=torch.int64, device="cuda")
        d_det = torch.zeros(2 * K, dtype=torch.int64, device="cuda")
        g.emit_device(n, d_rays.data_ptr(), d_state.data_ptr())
        if image:
            g.Image_device(n, n_bins, bin_len, FRAC, M, d_iwork.data_ptr(), d_hist.data_ptr(), d_det.data_ptr())
        g.receive_device(n, d_rays.data_ptr(), CASTS_OTHER, n_bins, bin_len, FRAC, d_state.data_ptr(), d_work.data_ptr(), d_last.data_ptr(),
                         d_hist.data_ptr(), d_det.data_ptr(), image=image)
        torch.cuda.synchronize()
        out[image] = dict(hist=d_hist.cpu().numpy().view(np.uint64).reshape(K, n_bins, B3), det=d_det.cpu().numpy().view(np.uint64).reshape(K, 2),
                          state=d_state.cpu().numpy().reshape(1 + B3, n), rays=d_rays.cpu().numpy(), last=d_last.cpu().numpy())
    got = out[True]
    assert (got["hist"] == want[0]).all() and (got["det"] == want[2]).all() and got["state"].tobytes() == want[3].tobytes()
    # the flag changes deposits only: final rays, state and the last events are those of the call without it
    for what in ("rays", "state", "last"):
        assert out[True][what].tobytes() == out[False][what].tobytes(), what
    assert (out[True]["hist"] != out[False]["hist"]).any()
