"""Developer tool: a long randomized differential run of the partition builders against the oracle -- tests.build_cases.sweep_case(seed),
the cases of tests/test_gpu_build_sweep.py, over any seed range.  On a machine with a GPU the device builders run (and, MODE=host, the
host builders); without one the host builders.  Lists, node arrays and the grid's geometry are compared for equality, a second build
byte for byte, a grid's shoot bit for bit.  Stops at the first difference, prints the seed with the first differing cell or node and
exits 1; nothing is tried twice.

    SEEDS=24:2000 python tools/fuzz_builders.py
    SEEDS=0:5000 MODE=host python tools/fuzz_builders.py
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hare_amd as H
from tests.build_cases import check_case, reference, sweep_case


def main():
    lo, hi = (int(x) for x in os.environ.get("SEEDS", "0:100").split(":"))
    host = os.environ.get("MODE", "") == "host" or H.device_count() == 0
    os.environ.pop("HARE_BUILD", None)
    t0 = time.time()
    for seed in range(lo, hi):
        case = sweep_case(seed)
        bad = check_case(case, reference(case), host=host)
        if bad:
            print("MISMATCH seed %d %s (%s): %s" % (seed, case.describe(), case.why, bad), flush=True)
            return 1
        print("seed %d clean (%s; %s), %.0f s" % (seed, case.describe(), case.why, time.time() - t0), flush=True)
    print("CLEAN: %s builders, seeds %d..%d, %.0f s" % ("host" if host else "device", lo, hi - 1, time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
