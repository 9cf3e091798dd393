"""Receiver maps on the MI355X at the edges of the visit rule (include/hare_hip.h, "Receiver maps"): every case of
tests.receive_map_ref.map_edge_cases() -- the exact layout h = 1, P = 0.625 with axis-parallel rays on and one ulp beyond the padded
faces, ties of the major axis with both signs, rays that only touch the padded grid, detections of receivers whose cell is never entered
(on each axis, as major and as minor axis), detections in the first and the last of ten slabs, q.q == r2; coplanar, collinear and
coincident centers, K = 1, a cell of 1/16 of the diameter, a cell that holds everything, one radius a hundred times the rest; grids of
128^3 and 2^21 x 1 x 1 cells crossed from outside; the layout scaled by 2^-20 and 2^30 and placed 0.999 x 2^20 cells from the origin;
directions scaled by 2^-30 .. 2^30 and 2^-600; and, outside the domain, rays with NaN, infinite, zero and denormal components, the
all-zero direction, directions scaled by 2^600 and a grid 2^50 m away that loses detections -- through Receive_batch and, for a subset,
receive_device and the sharded call over two scenes, compared byte for byte with the restatement (tests/receive_harness.py:
check_case).  Inside the domain, a map of K <= 256 receivers also gives the bytes of set_receivers.  A map of K = 936 on the exact pad
goes through Receive_batch_reduced (against tests/reduce_ref.py on the REFERENCE's histogram) and through Receive_source_reduced, plain
and with HARE_RECEIVE_DIRECT | HARE_RECEIVE_IMAGE (against reduce_ref on the plain call's histogram), four windows and the 31 decay
levels.  hare_receive_source with both flags, over that map and over the map 0.999 x 2^20 cells from the origin, equals
hist(no flag, b) - hist(no flag, 2) + direct + image with the two deposits from tests/direct_ref.py and tests/image_ref.py.
tests/test_receive_map_cases.py proves with the restatement alone that the cases hold these classes."""
import numpy as np
import pytest

from tests import direct_ref as dr
from tests import image_ref as ir
from tests.receive_cases import mesh_of, oracle_of, reference
from tests.receive_harness import check_case, library_partitions, mismatch, run_batch, same_bits
from tests.reduce_ref import reduce_ref
from tests.scatter_ref import normals_of
from tests.receive_map_ref import OUTSIDE, map_edge_cases

pytestmark = pytest.mark.gpu

CASES = map_edge_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_map_edge_case_equals_the_reference(case):
    want = reference(case, keep=True)
    assert want["det"][:, 0].sum() > 0, case.describe()
    seen = {}
    bad = check_case(case, want, seen=seen)
    note = {k: v for k, v in want["map_tallies"].items() if v}
    print(case.describe(), "tallies", note)
    assert seen["parts"][0].get_option("receiver_map") == 1
    assert bad is None, (case.describe(), bad, note)
    if case.device:
        assert seen["calls"] == [0, 0, 0], seen["calls"]
    if case.name not in OUTSIDE and case.K <= 256:                          # the identity: the same receivers through set_receivers
        hist, det, state = run_batch(case, library_partitions(case, linear=True))
        bad = mismatch(want, hist, det, state)
        assert bad is None, (case.describe(), "set_receivers " + bad)


# ---- K > 256 through the reduction and the source paths (tests/test_gpu_receive_reduced.py stops at K = 144)
WINDOWS = [(0, 64), (0, 7), (7, 64), (3, 40)]


def reduced_scene():
    import hare_amd as H
    case = next(c for c in CASES if c.name == "exact-half-K936")
    p = library_partitions(case)[0]
    p.set_source([3.875, 2.9375, 1.4375], power=[1.0, 0.5, 2.0]).set_option("source_seed", 21)
    return case, p, H.decay_levels(-np.arange(5.0, 36.0))


def test_batch_reduced_at_K936_is_the_reduction_of_the_references_histogram():
    case, p, levels = reduced_scene()
    want = reference(case, keep=True)
    sums, cross, det, state, _ = p.Receive_batch_reduced(case.rays, case.bounces, case.n_bins, case.bin_len, windows=WINDOWS, levels=levels,
                                                         frac_bits=case.frac_bits)
    want_sums, want_cross = reduce_ref(want["hist"], WINDOWS, levels, None)
    assert np.count_nonzero(want["hist"]) > 100 and len(np.unique(want_cross)) > 3
    for got, ref in ((sums, want_sums), (cross, want_cross), (det, want["det"]), (state, want["state"])):
        assert same_bits(got, ref) is None, same_bits(got, ref)


@pytest.mark.parametrize("flags", (dict(), dict(direct=True, image=True)), ids=("plain", "direct+image"))
def test_source_reduced_at_K936_is_the_reduction_of_the_plain_calls_histogram(flags):
    case, p, levels = reduced_scene()
    hist, _, det, state, ctr = p.Receive_source(4097, case.bounces, case.n_bins, case.bin_len, frac_bits=case.frac_bits, **flags)
    sums, cross, det2, state2, ctr2 = p.Receive_source_reduced(4097, case.bounces, case.n_bins, case.bin_len, windows=WINDOWS, levels=levels,
                                                               frac_bits=case.frac_bits, **flags)
    want_sums, want_cross = reduce_ref(hist, WINDOWS, levels, None)
    assert np.count_nonzero(hist) > 100 and (det[:, 0] > 0).sum() > 256 and len(np.unique(want_cross)) > 3
    for got, ref in ((sums, want_sums), (cross, want_cross), (det2, det), (state2, state)):
        assert same_bits(got, ref) is None, same_bits(got, ref)
    assert ctr2 == ctr
    if flags:                                                               # the flags are seen: cast 0 is the deposits, not detections
        assert (p.Receive_source(4097, case.bounces, case.n_bins, case.bin_len, frac_bits=case.frac_bits)[0] != hist).any()


# ---- the source paths over a map at these inputs: hist(DIRECT | IMAGE, b) = hist(0, b) - hist(0, 2) + direct + image, wrapping uint64
# (tests/test_gpu_direct.py: the flag replaces cast 0 by the deposit; tests/test_gpu_image.py: cast 1's specular detections by the images)
SOURCE = {"exact-half-K936": (3.875, 2.9375, 1.4375), "far-origin": (1047527.0 + 3.875, 1047527.0 + 2.9375, 1047527.0 + 1.4375)}
POWER = (1.0, 0.5, 2.0)


@pytest.mark.parametrize("name", SOURCE)
def test_source_with_direct_and_image_equals_the_identity_against_the_references(name):
    case = next(c for c in CASES if c.name == name).without(sigma=None, mode="specular")      # the identity holds without a scattering table
    p = library_partitions(case)[0]
    p.set_source(SOURCE[name], power=POWER).set_option("source_seed", 21)
    To, o = oracle_of(case)
    verts, nverts, _ = mesh_of(case.scene)
    n, K = 4097, case.K
    want_h, want_d = np.zeros((K, case.n_bins, 3), np.uint64), np.zeros((K, 2), np.uint64)
    dr.direct(o, SOURCE[name], POWER, None, 0, None, case.centers, case.radii, n, case.n_bins, case.bin_len, case.frac_bits, want_h, want_d)
    direct_found = int(want_d.sum())
    ir.image(o, verts, nverts, normals_of(To), SOURCE[name], POWER, None, 0, None, case.alpha, None, case.centers, case.radii, n, case.n_bins,
             case.bin_len, case.frac_bits, want_h, want_d)
    assert direct_found > 50 and int(want_d.sum()) - direct_found > 50          # both orders deposit
    call = lambda b, **f: p.Receive_source(n, b, case.n_bins, case.bin_len, frac_bits=case.frac_bits, **f)      # noqa: E731
    two = call(2)
    for bounces in (2, 3):
        plain = two if bounces == 2 else call(bounces)
        flag = call(bounces, direct=True, image=True)
        with np.errstate(over="ignore"):
            h, d = plain[0] - two[0] + want_h, plain[2] - two[2] + want_d
        assert same_bits(flag[0], h) is None, (name, bounces, same_bits(flag[0], h))
        assert same_bits(flag[2], d) is None, (name, bounces, same_bits(flag[2], d))
        assert flag[3].tobytes() == plain[3].tobytes() and flag[4] == plain[4]
    assert (call(3)[0] != two[0]).any()                                         # the third cast does detect
