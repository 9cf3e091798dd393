"""Developer tool: a long randomized differential run of the receive loop (hare_receive_batch and its sharded form) against the numpy
restatement -- tests.receive_cases.sweep_case(seed), the cases of tests/test_gpu_receive_sweep.py, over any seed range.  Histogram,
detections and final state are compared byte for byte (of a NaN, only that it is one).  Stops at the first difference, prints the case
that reproduces it and exits 1; nothing is tried twice.  With CUT=1 the termination rules (time limit, energy floor, roulette) are drawn
on top of every case, and every fourth seed also goes through receive_device: tests.receive_cut_ref.sweep_cut_case(seed), the cases of
tests/test_gpu_receive_cut.py's sweep.  With MAP=1 the cases are receiver maps, tests.receive_map_ref.map_sweep_case(seed), the cases of
tests/test_gpu_receive_map_sweep.py; every fourth seed also goes through receive_device.  The last line counts the device calls.

    SEEDS=200:2000 python tools/fuzz_receive.py
    CUT=1 SEEDS=40:2000 python tools/fuzz_receive.py
    MAP=1 SEEDS=100:600 python tools/fuzz_receive.py
"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.receive_cases import reference, sweep_case
from tests.receive_cut_ref import sweep_cut_case
from tests.receive_harness import check_case
from tests.receive_map_ref import map_sweep_case


def main():
    lo, hi = (int(x) for x in os.environ.get("SEEDS", "0:200").split(":"))
    cut = os.environ.get("CUT", "0") not in ("", "0")
    maps = os.environ.get("MAP", "0") not in ("", "0")
    what = "receiver maps" if maps else "receive loop with termination rules" if cut else "receive loop"
    t0 = time.time()
    calls = 0
    for seed in range(lo, hi):
        case = map_sweep_case(seed) if maps else sweep_cut_case(seed) if cut else sweep_case(seed)
        want = reference(case)
        device = (cut or maps) and seed % 4 == 0
        bad = check_case(case, want, device=device)
        calls += 1 + int(case.directional) + int(device) + int(case.two_scenes)
        if maps:
            note = "map tallies %s" % {k: v for k, v in want["map_tallies"].items() if v}
        elif cut:
            note = "retired %s" % {k: int(v.sum()) for k, v in want["per_cast"].items() if k != "live"}
        elif bad:
            note = "tallies %s" % {k: v for k, v in want["tallies"].items() if v}
        else:
            note = "detections %d binned %d not" % (int(want["det"][:, 0].sum()), int(want["det"][:, 1].sum()))
        if bad:
            print("MISMATCH seed %d %s: %s; %s" % (seed, case.describe(), bad, note), flush=True)
            return 1
        print("seed %d clean (%s), %s, %.0f s" % (seed, case.describe(), note, time.time() - t0), flush=True)
    print("CLEAN: %s, seeds %d..%d, %d device calls, %.0f s" % (what, lo, hi - 1, calls, time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
