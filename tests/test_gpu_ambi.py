"""The higher-order receivers on the MI355X (include/hare_hip.h, "receivers", "Higher orders": HARE_RECEIVE_ORDER2 and _ORDER3, nine and
sixteen channels per histogram word), byte for byte against tests/ambi_ref.py through tests/ambi_harness.py.

The scene cases: the 12-triangle shoebox, K = 3 with one receiver 2 m from the burst's source and one about it (many lanes of a wave in
one bin), 64 bins, four casts, n = 63 / 4 097 / 4 159, B = 1 / 3 / 8 (at B = 8 a bin holds 72 and 128 words, more than a wave has
lanes), both orders; "receive_aggregate" 1 and 0 return the same bytes.  Seeded scattering with the rain off and on; the three
partitions.  Then what the flags combine with: a map of 300 receivers against the linear loop on its first 256; HARE_RECEIVE_DIRECT,
_IMAGE and _IMAGE2 through the header's identities, word for word on every channel; the three source-path calls alone against the
reference deposit; chunks of a source burst and two scenes against the one call; the orders nested in one another; the numeric edges
(tests/ambi_cases.py: edge_case); the reduction on nine and sixteen channels."""
import dataclasses

import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests import ambi_cases as ac
from tests import ambi_ref
from tests import direct_ref as dr
from tests import image2_ref as i2
from tests import image_ref as ir
from tests import source_ref as sr
from tests.ambi_harness import check_case, library_partitions, run_batch, same_bits

pytestmark = pytest.mark.gpu

ORDERS = (2, 3)
FRAC = 40


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ---- the scene
@pytest.mark.parametrize("case", ac.scene_cases(), ids=lambda c: c.name)
def test_the_burst_in_the_shoebox_equals_the_reference_aggregated_or_not(case):
    want = ac.reference(case)
    assert want["det"][:, 0].min() > 0 and want["hist"][..., 4:].any(), case.describe()
    bad = check_case(case, want, device=case.n == 4159)
    assert bad is None, (case.describe(), bad)
    naive = dataclasses.replace(case, aggregate=0)
    bad = check_case(naive, want, device=False, lower=False)                    # "receive_aggregate" 0: every lane adds its own words
    assert bad is None, (naive.describe(), bad)


@pytest.mark.parametrize("case", ac.scatter_cases() + ac.partition_cases(), ids=lambda c: c.name)
def test_scattering_rain_and_the_three_partitions_equal_the_reference(case):
    want = ac.reference(case)
    assert want["det"][:, 0].min() > 0, case.describe()
    if case.mode == "rain":
        assert want["stats"]["eligible"] > 0
    bad = check_case(case, want, device=True)
    assert bad is None, (case.describe(), bad)


# ---- combinations
def test_a_map_of_300_receivers_equals_the_linear_loop_on_its_first_256():
    from tests.receive_map_ref import map_case
    mc = map_case("ambi-map300", "plane", 300, 4097, B=3, bounces=3, directional=True)
    case = ac.with_order(mc, 3)
    h, d, s = run_batch(case, library_partitions(case))
    assert h.shape == (300, case.n_bins, 3, 16)
    first = ac.with_order(mc, 3, centers=mc.centers[:256], radii=mc.radii[:256], map_cell=None)
    h0, d0, s0 = run_batch(first, library_partitions(first))
    assert d0[:, 0].sum() > 0 and h0[..., 4:].any() and d[256:, 0].sum() > 0
    for got, ref in ((h[:256], h0), (d[:256], d0), (s, s0)):
        assert same_bits(got, ref) is None, same_bits(got, ref)
    want = ac.reference(first)                                                  # and the linear loop is the definition
    assert same_bits(h0, want["hist"]) is None and same_bits(d0, want["det"]) is None


def widened(order, fn, shape4):
    """fn(hist, det) deposits into a four-channel histogram; returns (hist at `order`, det)."""
    hist, det = np.zeros(shape4, np.uint64), np.zeros((shape4[0], 2), np.uint64)
    with ambi_ref.higher_order(order) as extra:
        fn(hist, det)
    return ambi_ref.join(hist, extra), det


def image_terms(order, centers, radii, n, n_bins, bin_len):
    from tests.test_gpu_image import B3, PART, R3, SCENE, SRC, tables
    verts, nverts, _ = ir.mesh_of(SCENE)
    _, o, normals = ir.oracle_of(SCENE, PART)
    alpha, _ = tables()
    src = (SRC, sr.powers(B3), sr.rotation(), R3, sr.table(R3, B3))
    shape4 = (centers.shape[0], n_bins, B3, 4)
    first = widened(order, lambda h, d: ir.image(o, verts, nverts, normals, *src, alpha, None, centers, radii, n, n_bins, bin_len, FRAC, h, d), shape4)
    second = widened(order, lambda h, d: i2.image2(o, verts, nverts, normals, *src, alpha, None, centers, radii, n, n_bins, bin_len, FRAC, h, d), shape4)
    return first, second


@pytest.mark.parametrize("direct", (False, True), ids=("image+image2", "direct+image+image2"))
@pytest.mark.parametrize("order", ORDERS)
def test_the_image_flags_satisfy_the_headers_identity_on_every_channel(order, direct):
    """hist(flags) = hist - hist(bounces = 3) + hist(bounces = 1) + image + image2, word for word on all C channels."""
    from tests.test_gpu_image import scene_for
    g, centers, radii, kw, n_bins, bin_len = scene_for("directional")
    n = 4097
    (i_hist, i_det), (j_hist, j_det) = image_terms(order, centers, radii, n, n_bins, bin_len)
    assert int(i_det.sum()) > 0 and int(j_det.sum()) > 0 and i_hist[..., 4:].any() and j_hist[..., 4:].any()
    call = lambda bounces, flag: g.Receive_source(n, bounces, n_bins, bin_len, frac_bits=FRAC, direct=direct, image=flag, image2=flag, order=order, **kw)
    one, three = call(1, False), call(3, False)
    for bounces in (3, 5):
        plain = three if bounces == 3 else call(bounces, False)
        flag = call(bounces, True)
        with np.errstate(over="ignore"):
            want_h, want_d = plain[0] - three[0] + one[0] + i_hist + j_hist, plain[2] - three[2] + one[2] + i_det + j_det
        assert flag[0].shape[3] == ambi_ref.CHANNELS[order]
        assert (flag[0] == want_h).all(), (order, direct, bounces, np.argwhere(flag[0] != want_h)[:4])
        assert (flag[2] == want_d).all() and flag[3].tobytes() == plain[3].tobytes() and flag[4] == plain[4]


@pytest.mark.parametrize("order", ORDERS)
def test_the_direct_flag_satisfies_the_headers_identity_on_every_channel(order):
    """hist(HARE_RECEIVE_DIRECT) = hist - hist(bounces = 1) + the direct deposit; a one-cast call with the flag is the deposit alone."""
    from tests.test_gpu_direct import B3, R3, scene_for
    from tests.receive_cases import Case, oracle_of
    g, centers, radii, kw, n_bins, bin_len = scene_for("directional", False)
    _, o = oracle_of(Case("identity", ("room",), dr.PARTITIONS[0], np.zeros((0, 6)), 1, np.zeros((1, 3)), np.ones(1), 1, 1.0, 0))
    n = 4097
    d_hist, d_det = widened(order, lambda h, d: dr.direct(o, dr.POS, sr.powers(B3), sr.rotation(), R3, sr.table(R3, B3), centers, radii, n, n_bins,
                                                          bin_len, FRAC, h, d), (centers.shape[0], n_bins, B3, 4))
    assert int(d_det.sum()) > 0 and d_hist[..., 4:].any()
    first = g.Receive_source(n, 1, n_bins, bin_len, frac_bits=FRAC, order=order, **kw)
    for bounces in (1, 3):
        plain = first if bounces == 1 else g.Receive_source(n, bounces, n_bins, bin_len, frac_bits=FRAC, order=order, **kw)
        flag = g.Receive_source(n, bounces, n_bins, bin_len, frac_bits=FRAC, direct=True, order=order, **kw)
        with np.errstate(over="ignore"):
            assert (flag[0] == plain[0] - first[0] + d_hist).all(), (order, bounces, np.argwhere(flag[0] != plain[0] - first[0] + d_hist)[:4])
            assert (flag[2] == plain[2] - first[2] + d_det).all()
        if bounces == 1:
            assert (flag[0] == d_hist).all()


def _device_call(torch, g, words, K, work_bytes, call):
    """A source-path call onto random words with guards behind every buffer: (added histogram words, added detections)."""
    rng = np.random.default_rng(3)
    base_h = rng.integers(0, 2 ** 64, words + 64, dtype=np.uint64)
    base_d = rng.integers(0, 2 ** 64, 2 * K + 64, dtype=np.uint64)
    d_hist = torch.from_numpy(base_h.view(np.int64)).to("cuda")
    d_det = torch.from_numpy(base_d.view(np.int64)).to("cuda")
    d_work = torch.full((work_bytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    call(d_work.data_ptr(), d_hist.data_ptr(), d_det.data_ptr())
    torch.cuda.synchronize()
    hist, det, work = d_hist.cpu().numpy().view(np.uint64), d_det.cpu().numpy().view(np.uint64), d_work.cpu().numpy()
    assert (work[work_bytes:] == 0xA5).all() and (hist[words:] == base_h[words:]).all() and (det[2 * K:] == base_d[2 * K:]).all()
    with np.errstate(over="ignore"):
        return hist[:words] - base_h[:words], (det[:2 * K] - base_d[:2 * K]).reshape(K, 2)


@pytest.mark.parametrize("order", ORDERS)
def test_the_three_source_path_calls_alone_match_the_reference_deposit(torch, order):
    from tests.test_gpu_image import scene_for
    g, centers, radii, kw, n_bins, bin_len = scene_for("directional")
    n, K, B, C = 4097, centers.shape[0], 3, ambi_ref.CHANNELS[order]
    (i_hist, i_det), (j_hist, j_det) = image_terms(order, centers, radii, n, n_bins, bin_len)
    from tests.test_gpu_image import SCENE
    P = ir.mesh_of(SCENE)[0].shape[0]
    tail = (n, n_bins, bin_len, FRAC)
    words = K * n_bins * B * C
    h, d = _device_call(torch, g, words, K, H.Voxel_Grid.image_work_bytes(K, P, 1 << 16),
                        lambda dw, dh, dd: g.Image_device(*tail, 1 << 16, dw, dh, dd, directional=True, order=order))
    assert (h.reshape(i_hist.shape) == i_hist).all() and (d == i_det).all()
    h, d = _device_call(torch, g, words, K, H.Voxel_Grid.image2_work_bytes(P, 1 << 18, 1 << 16),
                        lambda dw, dh, dd: g.Image2_device(*tail, 1 << 18, 1 << 16, dw, dh, dd, directional=True, order=order))
    assert (h.reshape(j_hist.shape) == j_hist).all() and (d == j_det).all()
    # the direct sound on the same scene: the deposit of a one-cast call with the flag (identity above) is the call alone
    h, d = _device_call(torch, g, words, K, H.Voxel_Grid.direct_work_bytes(K),
                        lambda dw, dh, dd: g.direct_device(*tail, dw, dh, dd, directional=True, order=order))
    one = g.Receive_source(n, 1, n_bins, bin_len, frac_bits=FRAC, direct=True, directional=True, order=order)
    assert (h.reshape(one[0].shape) == one[0]).all() and (d == one[2]).all() and h.reshape(one[0].shape)[..., 4:].any()


# ---- additivity
@pytest.mark.parametrize("order", ORDERS)
def test_chunks_of_a_source_burst_and_two_scenes_sum_to_the_one_call(order):
    from tests.test_gpu_image import scene_for
    n = 4159
    g, centers, radii, kw, n_bins, bin_len = scene_for("directional", scatter=True)
    whole = g.Receive_source(n, 3, n_bins, bin_len, frac_bits=FRAC, directional=True, order=order)
    assert whole[2][:, 0].sum() > 0 and whole[0][..., 4:].any()
    chunks = [g.Receive_source(c, 3, n_bins, bin_len, first_ray=f, frac_bits=FRAC, directional=True, order=order) for f, c in ((0, 63), (63, 4034), (4097, 62))]
    with np.errstate(over="ignore"):
        assert (sum(c[0] for c in chunks) == whole[0]).all() and (sum(c[2] for c in chunks) == whole[2]).all()
    g2 = scene_for("directional", scatter=True)[0]
    two = H.Spatial_Partition.Receive_source_sharded([g, g2], n, 3, n_bins, bin_len, frac_bits=FRAC, directional=True, order=order)
    assert (two[0] == whole[0]).all() and (two[2] == whole[2]).all() and two[3].tobytes() == whole[3].tobytes()


# ---- edges
@pytest.mark.parametrize("case", ac.edge_cases(), ids=lambda c: c.name)
def test_the_numeric_edges_equal_the_reference(case):
    want = ac.reference(case)
    t = want["tallies"]
    assert want["det"][:, 0].sum() > 0 and t["saturated"] > 0 and t["zeroed_nan"] > 0, (case.describe(), t)
    assert t["dir_clamped"] > 0 and (case.frac_bits > 0 or t["ties"] > 0), (case.describe(), t)
    bad = check_case(case, want)
    assert bad is None, (case.describe(), bad)


# ---- reduction
@pytest.mark.parametrize("order", ORDERS)
def test_the_reduction_reads_word_0_of_nine_and_sixteen_channels(order):
    case = ac.burst_case(4097, 3, order)
    g = library_partitions(case)[0]
    hist, det, _ = run_batch(case, [g])
    spec = dict(windows=[(0, 64), (0, 8), (4, 40)], levels=[1 << 31, 1 << 28, 1 << 22])
    sums, cross = g.hist_reduce(hist, **spec)
    s0, c0 = g.hist_reduce(np.ascontiguousarray(hist[..., 0]), **spec)
    assert sums.any() and (sums == s0).all() and (cross == c0).all()


def test_receive_source_reduced_at_order_3_is_reduce_after_receive():
    from tests.test_gpu_image import scene_for
    g, centers, radii, kw, n_bins, bin_len = scene_for("directional")
    spec = dict(windows=[(0, n_bins), (0, 8)], levels=[1 << 31, 1 << 26])
    hist, _, det, state, ctr = g.Receive_source(4097, 3, n_bins, bin_len, frac_bits=FRAC, directional=True, order=3)
    sums, cross, det2, state2, ctr2 = g.Receive_source_reduced(4097, 3, n_bins, bin_len, frac_bits=FRAC, directional=True, order=3, **spec)
    s0, c0 = g.hist_reduce(hist, **spec)
    assert hist.shape[3] == 16 and sums.any()
    assert (sums == s0).all() and (cross == c0).all() and (det2 == det).all() and state2.tobytes() == state.tobytes() and ctr2 == ctr
