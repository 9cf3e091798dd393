"""Developer tool: a long randomized differential run of first-order edge diffraction (hare_diffract_device) against its numpy
restatement -- tests.diffract_cases.sweep_case(seed), the cases of tests/test_gpu_diffract.py's sweep, over any seed range.  Histogram,
detections, the pair count, the pair list as a set, the guards and the HIP call counters are compared as that module compares them.
Stops at the first difference, prints the seed that reproduces it and exits 1; nothing is tried twice.

    SEEDS=50:1000 python tools/fuzz_diffract.py
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tests.diffract_cases import reference, sweep_case
from tests.test_gpu_diffract import compare, run_device, scene_of


def main():
    lo, hi = (int(x) for x in os.environ.get("SEEDS", "50:150").split(":"))
    t0 = time.time()
    deposits = 0
    for seed in range(lo, hi):
        case = sweep_case(seed)
        want = reference(case)
        try:
            compare(case, want, *run_device(torch, scene_of(case), case, want["pairs"] + 3))
        except AssertionError as e:
            print("MISMATCH seed %d: %s" % (seed, str(e)[:400]), flush=True)
            return 1
        deposits += int(want["det"].sum())
    print("seeds %d .. %d clean, %d deposits compared, %.0f s" % (lo, hi - 1, deposits, time.time() - t0), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
