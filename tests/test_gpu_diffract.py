"""First-order edge diffraction on the MI355X (include/hare_hip.h, "receivers", "Edge diffraction (first order)").  hare_diffract_device
against tests/diffract_ref.py, byte for byte on the histogram and the detections and on the pair count, over tests/diffract_cases.py -- the
screen at B = 1, 3, 8, one to sixteen channels and the three partitions; the wedge, whose edges have two faces; the numeric edges (the apex
at an end, source and receiver on the edge's line, the apex inside the sphere, the detour at its limit and one ulp over, the limits 0 and
+inf, inv_lambda 0 and huge, the source inside a receiver, arrivals beyond the histogram, a directivity table); E = 1, 63, 65, 257 and
K = 257 through a receiver map -- accumulating onto a histogram that is not zero, with guard words behind every buffer untouched, the
three HIP call counters unmoved, a pair list of exactly the pairs found and both faces of the edge in the exclusion words of both legs.  The list one pair short (nothing added, the count reported,
HARE_E_NOMEM from the host call); the call twice (every word doubled); the host call against the device call; the screen's receivers get
words from the direct sound or from diffraction, never from both; a sweep of 50 drawn scenes."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests import diffract_cases as dc
from tests.receive_harness import CALL_COUNTERS

pytestmark = pytest.mark.gpu

GUARD = 64                                   # bytes behind d_work; 8-byte words behind d_hist and d_detections
FILL = 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def scene_of(case):
    verts, nverts = case.geometry()
    T = H.Topology(verts, nverts)
    kind, *par = case.partition
    g = H.Voxel_Grid([T], par[0]) if kind == "voxel" else (H.Octree if kind == "octree" else H.KDTree)([T], *par)
    (g.set_receiver_map if case.map else g.set_receivers)(case.centers, case.radii)
    if case.B > 1:
        g.set_absorption(np.zeros((T.Polygon_Count, case.B)))            # the topology's band count: the source's must be the same
    pos, power, frame, R, gain = case.source()
    g.set_source(pos, power=power, frame=frame, gain=gain)
    g.set_edges(case.ends, case.faces, case.inv_lambda)
    return g


def device_u64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1)).to("cuda")


def run_device(torch, g, case, max_pairs, times=1):
    """hare_diffract_device of the case onto random words, `times` times: (added histogram, added detections, pairs found, the list's
    (k, j) rows)."""
    K, words = case.K, int(np.prod(case.shape))
    rng = np.random.default_rng(3)
    base_h = rng.integers(0, 2 ** 64, words + GUARD, dtype=np.uint64)           # the call ACCUMULATES: onto words that are not zero
    base_d = rng.integers(0, 2 ** 64, 2 * K + GUARD, dtype=np.uint64)
    d_hist, d_det = device_u64(torch, base_h), device_u64(torch, base_d)
    wb = H.Voxel_Grid.diffract_work_bytes(K, max_pairs)
    d_work = torch.full((wb + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = [g.get_option(o) for o in CALL_COUNTERS]
    for _ in range(times):
        g.diffract_device(case.n_weight, case.n_bins, case.bin_len, case.frac_bits, max_pairs, d_work.data_ptr(), d_hist.data_ptr(), d_det.data_ptr(),
                          max_detour=case.max_detour, directional=case.order > 0, order=max(case.order, 1))
    after = [g.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    assert after == before, dict(zip(CALL_COUNTERS, (a - b for a, b in zip(after, before))))
    hist, det, work = d_hist.cpu().numpy().view(np.uint64), d_det.cpu().numpy().view(np.uint64), d_work.cpu().numpy()
    assert (work[wb:] == FILL).all() and (hist[words:] == base_h[words:]).all() and (det[2 * K:] == base_d[2 * K:]).all()
    found = int(work[:8].view(np.uint64)[0])
    S = K + 2 * max_pairs                                                      # the shadow slots: rays, t_max, then the two exclusion words
    kj = work[256 + 68 * S:][:8 * max_pairs].view(np.int32).reshape(max_pairs, 2)
    excl = work[256 + 56 * S:][:8 * S].view(np.int32).reshape(2, S)[:, K:].reshape(2, max_pairs, 2)
    if found <= max_pairs:                                                       # both legs of a pair carry both faces of its edge
        want = np.asarray(case.faces, np.int32)[kj[:found, 1]]
        assert (excl[0, :found] == want[:, :1]).all() and (excl[1, :found] == want[:, 1:]).all()
        assert (excl[0, found:] == -2).all()                                    # the slots without a pair are marked: no query
    with np.errstate(over="ignore"):
        return ((hist[:words] - base_h[:words]).reshape(case.shape), (det[:2 * K] - base_d[:2 * K]).reshape(K, 2), found,
                kj[:min(found, max_pairs)].copy())


def compare(case, want, got_h, got_d, found, kj):
    s = want["seen"]
    print(case.name, "pairs", want["pairs"], "deposited", int(want["det"].sum()), "words", int((want["hist"] != 0).sum()))
    assert found == want["pairs"]
    assert sorted(map(tuple, kj.tolist())) == sorted(zip(s["k"].tolist(), s["j"].tolist()))          # the list, as a set
    bad = np.argwhere(got_d != want["det"])
    assert bad.size == 0, (bad[:4], got_d[tuple(bad[0])], want["det"][tuple(bad[0])])
    bad = np.argwhere(got_h != want["hist"])
    assert bad.size == 0, (len(bad), bad[:4], got_h[tuple(bad[0])], want["hist"][tuple(bad[0])])


@pytest.mark.parametrize("case", dc.cases(), ids=lambda c: c.name)
def test_diffract_device_matches_the_reference(torch, case):
    want = dc.reference(case)
    compare(case, want, *run_device(torch, scene_of(case), case, max(1, want["pairs"])))      # a list of exactly the pairs there are


@pytest.mark.parametrize("seed", dc.SWEEP)
def test_sweep(torch, seed):
    case = dc.sweep_case(seed)
    want = dc.reference(case)
    compare(case, want, *run_device(torch, scene_of(case), case, want["pairs"] + 3))


def test_a_list_one_pair_short_adds_nothing_and_reports_the_count(torch):
    case = dc.case_named("screen-B3-dir")
    want = dc.reference(case)
    g = scene_of(case)
    got_h, got_d, found, _ = run_device(torch, g, case, want["pairs"] - 1)
    assert found == want["pairs"] and not got_h.any() and not got_d.any()
    with pytest.raises(H.HareError) as e:
        g.Diffract_paths(case.n_weight, case.n_bins, case.bin_len, want["pairs"] - 1, frac_bits=case.frac_bits, directional=True)
    assert e.value.code == capi.HARE_E_NOMEM and e.value.found == want["pairs"] and str(want["pairs"]) in str(e.value)


@pytest.mark.parametrize("name", ("screen-B3-dir", "wedge-B3"))
def test_the_call_twice_doubles_every_word(torch, name):
    case = dc.case_named(name)
    want = dc.reference(case)
    got_h, got_d, found, _ = run_device(torch, scene_of(case), case, want["pairs"], times=2)
    with np.errstate(over="ignore"):
        assert found == want["pairs"] and (got_h == want["hist"] * np.uint64(2)).all() and (got_d == want["det"] * np.uint64(2)).all()
    assert want["hist"].any()


@pytest.mark.parametrize("name", ("screen-B1", "screen-B8-dir2", "wedge-B8-kdtree", "size-K257-map"))
def test_the_host_call_is_the_device_call_on_zeros(name):
    case = dc.case_named(name)
    want = dc.reference(case)
    hist, det, found = scene_of(case).Diffract_paths(case.n_weight, case.n_bins, case.bin_len, want["pairs"] + 1, frac_bits=case.frac_bits,
                                                      max_detour=case.max_detour, directional=case.order > 0, order=max(case.order, 1))
    assert found == want["pairs"] and (hist == want["hist"]).all() and (det == want["det"]).all()


def test_a_receiver_hears_the_direct_sound_or_the_diffracted_one_never_both(torch):
    case = dc.case_named("screen-B1")
    g = scene_of(case)
    hist, det, _ = g.Diffract_paths(case.n_weight, case.n_bins, case.bin_len, 64, frac_bits=case.frac_bits)
    d_hist, d_det = g.Source_paths(case.n_weight, case.n_bins, case.bin_len, frac_bits=case.frac_bits, image=False, image2=False)
    direct, bent = d_det.sum(axis=1) > 0, det.sum(axis=1) > 0
    assert not (direct & bent).any() and direct.any() and bent.any()
    assert (hist.reshape(case.K, -1).any(axis=1) == bent).all() and (d_hist.reshape(case.K, -1).any(axis=1) == direct).all()
