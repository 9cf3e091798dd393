"""The source paths on the MI355X at ambisonic orders 2 and 3 -- the nine- and sixteen-channel forms of the three deposits
(hare_direct_device, hare_image_device, hare_image2_device with HARE_RECEIVE_ORDER2 / _ORDER3) -- through
tests.path_harness.check_case against tests.path_cases.reference: histogram and detections byte for byte on every channel, the counts, the
lists as sets, the guards, the HIP call counters.

The fixed cases, tests.path_cases.ambi_edge_cases(): every directional case of tests/test_gpu_path_edges.py again at both orders, in its
oblique room; arrivals along the axes, the face diagonals and the space diagonals of an unmapped box, with az == 0 and Y6 == -0.5
exactly; m = 1, 3, 5 at frac_bits 0 and 1 (ties of the signed words) and m = 2^63 at frac_bits 62 (the clamp); B = 8 at order 3, 128
words per deposit, at K = 255, 256 and 257 and at P = 256 with the second order; more than 50 first-order and 200 second-order paths
of a receiver in one bin; order 3 under every partition.  A case that carries an option pair runs with 0 and with 1.
tests/test_path_cases.py asserts on the CPU that each case holds the class it names.

The sweep: tests.path_cases.ambi_sweep_case(seed) for seeds 0 .. N - 1 -- tests/test_gpu_path_sweep.py's case of the seed, directional, at
a drawn order 2 or 3, n_bins halved and bin_len doubled until the words fit, K cut where B x C is large, and a histogram that ends
before the nearest receiver (nothing could be binned) lengthened past the farthest (the rules are ambi_sweep_case's docstring).  No seed
is skipped or redrawn; 8 of the 100 leave the channels 4 .. C - 1 all zero.  tools/fuzz_paths.py --ambi runs the same cases over any
seed range.

N = 100.  On an MI355X host this module alone, reference side included, takes 31.9 s of wall time (149 passed; 16 threads); its slowest
tests are the K = 255 .. 257 cases at B = 8 and order 3 and P255-K8-second-o2, 1 to 2 s each.  The reference side of the 100 seeds alone
takes about 67 s on a slow 16-thread CPU host where tests/test_gpu_path_sweep.py's takes 40 s (under twice that: N stays 100); the fixed
cases' reference side takes 30 s there."""
import pytest

from tests.path_cases import ambi_edge_cases, ambi_sweep_case, reference, variants
from tests.path_harness import check_case

pytestmark = pytest.mark.gpu

N = 100
RUNS = [v for c in ambi_edge_cases() for v in variants(c)]


@pytest.mark.parametrize("case", RUNS, ids=[c.name + "".join(f"-{o.split('_')[1]}{getattr(c, o)}" for o in c.pair) for c in RUNS])
def test_ambi_edge_case_equals_the_reference(case):
    want = reference(case, keep=True)                                   # the options do not enter the reference: one result per name
    bad = check_case(case, want)
    assert bad is None, (case.describe(), case.why, bad)


@pytest.mark.parametrize("seed", range(N))
def test_ambi_sweep_seed_equals_the_reference(seed):
    case = ambi_sweep_case(seed)
    want = reference(case)
    assert sum(int(w["det"].sum()) for w in want.values()) > 0, case.describe()
    bad = check_case(case, want)
    assert bad is None, (case.describe(), bad)
