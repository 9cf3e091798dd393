"""Developer tool: a long randomized differential run of the source paths (hare_direct_device, hare_image_device, hare_image2_device)
against their numpy restatements -- tests.path_cases.sweep_case(seed), the cases of tests/test_gpu_path_sweep.py, over any seed range.
Histogram and detections are compared byte for byte, the counts, the lists as sets, the guards and the HIP call counters as
tests.path_harness.check_case compares them.  Stops at the first difference, prints the case that reproduces it and exits 1; nothing is
tried twice.  --ambi runs tests.path_cases.ambi_sweep_case(seed) instead, the cases of tests/test_gpu_path_ambi.py: the same seeds at
ambisonic order 2 or 3, nine or sixteen channels.

    SEEDS=100:1000 python tools/fuzz_paths.py [--ambi]
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.path_cases import ambi_sweep_case, reference, sweep_case
from tests.path_harness import check_case


def main():
    lo, hi = (int(x) for x in os.environ.get("SEEDS", "0:100").split(":"))
    case_of = ambi_sweep_case if "--ambi" in sys.argv[1:] else sweep_case
    t0 = time.time()
    compared = 0
    for seed in range(lo, hi):
        case = case_of(seed)
        want = reference(case)
        bad = check_case(case, want)
        note = " ".join("%s %d" % (o, int(w["det"].sum())) for o, w in want.items())
        if bad:
            print("MISMATCH seed %d %s: %s; deposits %s" % (seed, case.describe(), bad, note), flush=True)
            return 1
        compared += len(case.orders)
        print("seed %d clean (%s), deposits %s, %.0f s" % (seed, case.describe(), note, time.time() - t0), flush=True)
    print("CLEAN: source paths, seeds %d..%d, %d device calls compared, %.0f s" % (lo, hi - 1, compared, time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
