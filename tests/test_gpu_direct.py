"""The direct sound on the MI355X (include/hare_hip.h, "receivers", "Direct sound").  hare_direct_device against tests/direct_ref.py, byte
for byte on the histogram and the detections, over direct_ref.cases() -- the three partitions in the partition room, whose wall hides
some receivers; K = 1 .. 256 linear, 257 and 4 096 as a map; B = 1, 3, 8; no table and two resolutions in a rotated frame; frac_bits 0,
40, 62; one bin and 4 096; one and four channels; n_weight 1, 4 097, 2^40 -- accumulating onto a histogram that is not zero, with guard
words behind every buffer untouched and the three HIP call counters unmoved.  The identity

    hist(flag, bounces) = hist(no flag, bounces) - hist(no flag, bounces = 1) + direct          (wrapping uint64; detections alike)

on hare_receive_source in every mode of the loop, over the linear receivers and a map, with state and counters equal with and without the
flag; the sharded call over two scenes (the deposit is made once); the reduced call; and hare_receive_device with the flag plus
hare_direct_device, which together reproduce hare_receive_source with the flag."""
import numpy as np
import pytest

import hare_amd as H
from tests import direct_ref as dr
from tests import source_ref as sr
from tests.receive_cases import Case, alpha_table, mesh_of, oracle_of, sigma_table
from tests.receive_harness import CALL_COUNTERS

pytestmark = pytest.mark.gpu

GUARD = 64                                   # bytes behind d_work; 8-byte words behind d_hist and d_detections
FILL = 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def library_partition(partition, scene=("room",)):
    verts, nverts, _ = mesh_of(scene)
    T = H.Topology(verts, nverts)
    kind, *par = partition
    return H.Voxel_Grid([T], par[0]) if kind == "voxel" else (H.Octree if kind == "octree" else H.KDTree)([T], *par), T


def device_u64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1)).to("cuda")


# ---- hare_direct_device against the reference
@pytest.mark.parametrize("case", dr.cases(), ids=lambda c: c.name)
def test_direct_device_matches_the_reference(torch, case):
    want = dr.reference(case)
    g, T = library_partition(case.partition, case.scene)
    centers, radii = case.receivers()
    (g.set_receiver_map if case.map else g.set_receivers)(centers, radii)
    if case.B > 1:
        g.set_absorption(np.zeros((T.Polygon_Count, case.B)))                   # fixes the topology's B
    pos, power, frame, R, gain = case.source()
    g.set_source(pos, power=power, frame=frame, gain=gain)
    K, words = case.K, int(np.prod(case.shape))
    rng = np.random.default_rng(3)
    base_h = rng.integers(0, 2 ** 64, words + GUARD, dtype=np.uint64)           # the call ACCUMULATES: onto words that are not zero
    base_d = rng.integers(0, 2 ** 64, 2 * K + GUARD, dtype=np.uint64)
    d_hist, d_det = device_u64(torch, base_h), device_u64(torch, base_d)
    wb = H.Voxel_Grid.direct_work_bytes(K)
    d_work = torch.full((wb + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = [g.get_option(o) for o in CALL_COUNTERS]
    g.direct_device(case.n_weight, case.n_bins, case.bin_len, case.frac_bits, d_work.data_ptr(), d_hist.data_ptr(), d_det.data_ptr(),
                    directional=case.directional)
    after = [g.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    assert after == before, dict(zip(CALL_COUNTERS, (a - b for a, b in zip(after, before))))
    hist, det = d_hist.cpu().numpy().view(np.uint64), d_det.cpu().numpy().view(np.uint64)
    assert (d_work.cpu().numpy()[wb:] == FILL).all() and (hist[words:] == base_h[words:]).all() and (det[2 * K:] == base_d[2 * K:]).all()
    with np.errstate(over="ignore"):
        got_d = (det[:2 * K] - base_d[:2 * K]).reshape(K, 2)
        got_h = (hist[:words] - base_h[:words]).reshape(case.shape)
    print(case.name, "visible", int(want["det"].sum()), "occluded", int(want["seen"]["occluded"].sum()), "words", int((want["hist"] != 0).sum()))
    bad = np.argwhere(got_d != want["det"])
    assert bad.size == 0, (bad[:4], got_d[tuple(bad[0])], want["det"][tuple(bad[0])])
    bad = np.argwhere(got_h != want["hist"])
    assert bad.size == 0, (len(bad), bad[:4], got_h[tuple(bad[0])], want["hist"][tuple(bad[0])])


# ---- the identity on hare_receive_source
B3, R3, FRAC = 3, 4, 30
MODES = ("specular", "scatter", "rain", "directional", "cut")
SIZES, CASTS = (1, 65, 4097), (1, 2, 5)


def receivers_of(as_map):
    c = dr.DirectCase("identity", dr.PARTITIONS[0], 300 if as_map else 6, as_map, B3, R3, FRAC, 64, 0.25, False, 1)
    return c.receivers()


def scene_for(mode, as_map, partition=dr.PARTITIONS[0]):
    """The partition room with three bands of absorption (and scattering in the modes that scatter), a directional source at direct_ref.POS
    and receivers on both sides of the wall: the library partition, and what the calls of this mode take."""
    g, T = library_partition(partition)
    rng = np.random.default_rng(9)
    centers, radii = receivers_of(as_map)
    (g.set_receiver_map if as_map else g.set_receivers)(centers, radii)
    g.set_absorption(alpha_table(T.Polygon_Count, B3, rng))
    if mode in ("scatter", "rain", "cut"):
        g.set_scattering(sigma_table(T.Polygon_Count, B3, rng)).set_option("scatter_seed", 5)
    if mode == "cut":
        g.set_option("receive_floor_bits", 2).set_option("receive_roulette", 1)
    g.set_source(dr.POS, power=sr.powers(B3), frame=sr.rotation(), gain=sr.table(R3, B3)).set_option("source_seed", 21)
    kw = dict(rain=mode == "rain", directional=mode == "directional", time_limit=mode == "cut")
    n_bins, bin_len = (24, 0.25) if mode == "cut" else (64, 0.25)                # the time limit bites: 6 m of histogram
    return g, centers, radii, kw, n_bins, bin_len


def direct_term(centers, radii, n, n_bins, bin_len, directional, partition=dr.PARTITIONS[0]):
    _, o = oracle_of(Case("identity", ("room",), partition, np.zeros((0, 6)), 1, np.zeros((1, 3)), np.ones(1), 1, 1.0, 0))
    K = centers.shape[0]
    hist = np.zeros((K, n_bins, B3, 4) if directional else (K, n_bins, B3), np.uint64)
    det = np.zeros((K, 2), np.uint64)
    dr.direct(o, dr.POS, sr.powers(B3), sr.rotation(), R3, sr.table(R3, B3), centers, radii, n, n_bins, bin_len, FRAC, hist, det)
    return hist, det


# rain does not combine with a map (HARE_E_INVALID): every other pairing
@pytest.mark.parametrize("mode,as_map", [(m, a) for m in MODES for a in (False, True) if not (m == "rain" and a)],
                         ids=lambda v: v if isinstance(v, str) else ("map" if v else "linear"))
def test_the_flag_replaces_cast_0_by_the_deposit(mode, as_map):
    g, centers, radii, kw, n_bins, bin_len = scene_for(mode, as_map)
    deposits = 0
    for n in SIZES:
        d_hist, d_det = direct_term(centers, radii, n, n_bins, bin_len, kw["directional"])
        deposits += int(d_det.sum())
        first = g.Receive_source(n, 1, n_bins, bin_len, frac_bits=FRAC, **kw)
        for bounces in CASTS:
            plain = first if bounces == 1 else g.Receive_source(n, bounces, n_bins, bin_len, frac_bits=FRAC, **kw)
            flag = g.Receive_source(n, bounces, n_bins, bin_len, frac_bits=FRAC, direct=True, **kw)
            tag = (mode, as_map, n, bounces)
            with np.errstate(over="ignore"):
                assert (flag[0] == plain[0] - first[0] + d_hist).all(), (tag, np.argwhere(flag[0] != plain[0] - first[0] + d_hist)[:4])
                assert (flag[2] == plain[2] - first[2] + d_det).all(), tag
            assert flag[3].tobytes() == plain[3].tobytes() and flag[4] == plain[4], tag          # state and counters
            if bounces == 1:
                assert (flag[0] == d_hist).all(), tag                            # a one-cast call with the flag is the deposit alone
            if kw["directional"]:
                omni = g.Receive_source(n, bounces, n_bins, bin_len, frac_bits=FRAC, direct=True, **dict(kw, directional=False))
                assert (flag[0][..., 0] == omni[0]).all() and (flag[2] == omni[2]).all(), tag
    assert deposits > 0 and first[0].any()                                       # something was deposited, and cast 0 does detect without the flag


# ---- the other calls
N_OTHER, CASTS_OTHER = 4097, 3


def test_sharded_over_two_scenes_deposits_once():
    a, centers, radii, kw, n_bins, bin_len = scene_for("scatter", False)
    b = scene_for("scatter", False)[0]
    for n in (N_OTHER, 1):                                                       # n = 1: scenes[0]'s shard is empty, scenes[1] deposits
        one = a.Receive_source(n, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, direct=True)
        two = H.Spatial_Partition.Receive_source_sharded([a, b], n, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, direct=True)
        assert (one[0] == two[0]).all() and (one[2] == two[2]).all() and one[3].tobytes() == two[3].tobytes() and one[4] == two[4], n
        assert one[2].sum() > 0


def test_reduced_with_the_flag_is_the_reduction_of_the_flagged_histogram():
    g, centers, radii, kw, n_bins, bin_len = scene_for("specular", True)
    spec = dict(windows=[(0, n_bins), (0, 8), (8, n_bins)], levels=H.decay_levels([-5, -10]).tolist())
    hist, _, det, state, ctr = g.Receive_source(N_OTHER, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, direct=True)
    sums, cross, det2, state2, ctr2 = g.Receive_source_reduced(N_OTHER, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, direct=True, **spec)
    want_sums, want_cross = g.hist_reduce(hist, **spec)
    assert (sums == want_sums).all() and (cross == want_cross).all() and (det == det2).all() and state.tobytes() == state2.tobytes() and ctr == ctr2
    plain = g.Receive_source_reduced(N_OTHER, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, **spec)
    assert (plain[0] != sums).any()                                              # the flag is seen


@pytest.mark.parametrize("as_map", (False, True), ids=("linear", "map"))
def test_receive_device_with_the_flag_and_direct_device_reproduce_receive_source(torch, as_map):
    g, centers, radii, kw, n_bins, bin_len = scene_for("scatter", as_map, dr.PARTITIONS[2])
    n, K = N_OTHER, centers.shape[0]
    want = g.Receive_source(n, CASTS_OTHER, n_bins, bin_len, frac_bits=FRAC, direct=True)
    out = {}
    for direct in (True, False):
        d_rays = torch.empty(n * 6, dtype=torch.float64, device="cuda")
        d_state = torch.empty(n * (1 + B3), dtype=torch.float64, device="cuda")
        d_work = torch.zeros(H.Voxel_Grid.receive_work_bytes(n), dtype=torch.uint8, device="cuda")
        d_dwork = torch.zeros(H.Voxel_Grid.direct_work_bytes(K), dtype=torch.uint8, device="cuda")
        d_last = torch.zeros(n * 56, dtype=torch.uint8, device="cuda")
        d_hist = torch.zeros(K * n_bins * B3, dtype=torch.int64, device="cuda")
        d_det = torch.zeros(2 * K, dtype=torch.int64, device="cuda")
        g.emit_device(n, d_rays.data_ptr(), d_state.data_ptr())
        if direct:
            g.direct_device(n, n_bins, bin_len, FRAC, d_dwork.data_ptr(), d_hist.data_ptr(), d_det.data_ptr())
        g.receive_device(n, d_rays.data_ptr(), CASTS_OTHER, n_bins, bin_len, FRAC, d_state.data_ptr(), d_work.data_ptr(), d_last.data_ptr(),
                         d_hist.data_ptr(), d_det.data_ptr(), direct=direct)
        torch.cuda.synchronize()
        out[direct] = dict(hist=d_hist.cpu().numpy().view(np.uint64).reshape(K, n_bins, B3), det=d_det.cpu().numpy().view(np.uint64).reshape(K, 2),
                           state=d_state.cpu().numpy().reshape(1 + B3, n), rays=d_rays.cpu().numpy(), last=d_last.cpu().numpy())
    got = out[True]
    assert (got["hist"] == want[0]).all() and (got["det"] == want[2]).all() and got["state"].tobytes() == want[3].tobytes()
    # the flag changes deposits only: final rays, state and the last events are those of the call without it
    for what in ("rays", "state", "last"):
        assert out[True][what].tobytes() == out[False][what].tobytes(), what
    assert (out[True]["hist"] != out[False]["hist"]).any()
