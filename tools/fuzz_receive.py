"""Developer tool: a long randomized differential run of the receive loop (hare_receive_batch and its sharded form) against the numpy
restatement -- tests.receive_cases.sweep_case(seed), the cases of tests/test_gpu_receive_sweep.py, over any seed range.  Histogram,
detections and final state are compared byte for byte (of a NaN, only that it is one).  Stops at the first difference, prints the case
that reproduces it and exits 1; nothing is tried twice.  With CUT=1 the termination rules (time limit, energy floor, roulette) are drawn
on top of every case: tests.receive_cut_ref.sweep_cut_case(seed), the cases of tests/test_gpu_receive_cut.py's sweep.

    SEEDS=200:2000 python tools/fuzz_receive.py
    CUT=1 SEEDS=40:2000 python tools/fuzz_receive.py
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.receive_cases import reference, sweep_case
from tests.test_gpu_receive_edges import check_case


def main_cut(lo, hi):
    from tests.receive_cut_ref import reference as cut_reference, sweep_cut_case
    from tests.test_gpu_receive_cut import check_case as check_cut_case
    t0 = time.time()
    for seed in range(lo, hi):
        cc = sweep_cut_case(seed)
        want = cut_reference(cc, keep=False)
        bad = check_cut_case(cc, want, device=seed % 4 == 0)
        retired = {k: int(v.sum()) for k, v in want["per_cast"].items() if k != "live"}
        if bad:
            print("MISMATCH seed %d %s: %s; retired %s" % (seed, cc.describe(), bad, retired), flush=True)
            return 1
        print("seed %d clean (%s), retired %s, %.0f s" % (seed, cc.describe(), retired, time.time() - t0), flush=True)
    print("CLEAN: receive loop with termination rules, seeds %d..%d, %.0f s" % (lo, hi - 1, time.time() - t0))
    return 0


def main():
    lo, hi = (int(x) for x in os.environ.get("SEEDS", "0:200").split(":"))
    if os.environ.get("CUT", "0") not in ("", "0"):
        return main_cut(lo, hi)
    t0 = time.time()
    for seed in range(lo, hi):
        case = sweep_case(seed)
        want = reference(case)
        bad = check_case(case, want)
        if bad:
            print("MISMATCH seed %d %s: %s; tallies %s" % (seed, case.describe(), bad, {k: v for k, v in want["tallies"].items() if v}), flush=True)
            return 1
        print("seed %d clean (%s), detections %d binned %d not, %.0f s" % (seed, case.describe(), int(want["det"][:, 0].sum()),
                                                                         int(want["det"][:, 1].sum()), time.time() - t0), flush=True)
    print("CLEAN: receive loop, seeds %d..%d, %.0f s" % (lo, hi - 1, time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
