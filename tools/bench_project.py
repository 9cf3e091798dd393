"""Cost of the histogram projection (include/hare_hip.h, "receivers", "Projection"; kernel hare_hist_project, project.hip) beside the
reduction and beside the copy it replaces.  A developer tool; needs an MI355X and torch.

For each shape (default: K = 16 384, n_bins = 1 024, B = 8 -- the 1 GiB cap -- and K = 1 024, n_bins = 4 000, B = 8) a device histogram
is filled from a seed and hare_hist_project_device is timed for J = 1, 8 and 29 vectors (--vectors), without and with weights: device
events around one call, a warm-up first, the median of --reps (default 25, at least 20) and the spread.  The coefficients are the STI
table of hare_amd.sti.mtf_vectors (ones, cosines, sines), cut to J rows.  In the same run, as yardsticks: hare_hist_reduce_device with 4
windows and no levels on the same histogram, and the device-to-pinned-host copy of the histogram (median of --copy-reps).  Printed, one
JSON object per line: the times in ms; for each projection its ratio to both yardsticks (time / reduce, copy / time); hbm_fraction, the
histogram's bytes COUNTED ONCE over the kernel's time as a fraction of the 8 TB/s HBM peak (a sweep per eight vectors reads the block
again, expected from L2: not counted); and per shape and weights the cost per added vector, (t(J_max) - t(J_min)) / (J_max - J_min).
One result is checked against the integer restatement on receiver 0 before anything is timed.

  python tools/bench_project.py [--reps 25] [--copy-reps 7] [--shapes 16384x1024x8,1024x4000x8] [--vectors 1,8,29]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hare_amd as H  # noqa: E402
from hare_amd import sti  # noqa: E402

HBM_PEAK = 8.0e12


def events_ms(torch, fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), n=len(ms))


def exact(hist, coef, weight):
    """The definition on one receiver in Python integers: [B][J]."""
    g = hist.tolist() if weight is None else [[(h * w) >> 32 for h, w in zip(hr, wr)] for hr, wr in zip(hist.tolist(), weight.tolist())]
    return [[sum(int(c) * row[b] for c, row in zip(cj, g)) for cj in coef.tolist()] for b in range(hist.shape[1])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--copy-reps", type=int, default=7)
    ap.add_argument("--shapes", default="16384x1024x8,1024x4000x8")
    ap.add_argument("--vectors", default="1,8,29")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    if H.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("bench_project: no GPU -- there is nothing to measure without one")
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    stream = torch.cuda.current_stream().cuda_stream
    vectors = [int(x) for x in a.vectors.split(",")]
    for shape in a.shapes.split(","):
        K, n_bins, B = (int(x) for x in shape.split("x"))
        words = K * n_bins * B
        gen = torch.Generator(device="cuda").manual_seed(7)
        d_hist = torch.randint(0, 1 << 40, (words,), dtype=torch.int64, device="cuda", generator=gen)
        weight = H.air_weights(np.linspace(0.001, 0.02, B), 0.01, n_bins)
        d_weight = torch.from_numpy(weight.view(np.int32)).to("cuda")
        table = sti.mtf_vectors(n_bins, 0.01, 1.0)                       # 29 x n_bins: 10 ms bins
        d_coef = torch.from_numpy(table).to("cuda")
        d_proj = torch.zeros(K * B * max(vectors) * 2, dtype=torch.int64, device="cuda")
        # receiver 0 against the definition, J = max, with weights
        J = max(vectors)
        g.hist_project_device(K, n_bins, B, 1, d_hist.data_ptr(), J, d_coef.data_ptr(), d_proj.data_ptr(), d_weight=d_weight.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        got = H.proj_to_int(d_proj[:B * J * 2].cpu().numpy().view(np.uint64).reshape(B, J, 2)).tolist()
        want = exact(d_hist[:n_bins * B].cpu().numpy().view(np.uint64).reshape(n_bins, B), table[:J], weight)
        if got != want:
            raise SystemExit("bench_project: receiver 0 differs from the definition")
        # yardstick 1: the reduction, 4 windows, no levels
        windows = [(0, n_bins), (0, n_bins // 20), (0, n_bins // 12), (n_bins // 12, n_bins)]
        d_sums = torch.zeros(K * B * len(windows) * 4, dtype=torch.int64, device="cuda")
        reduce_ms = {}
        for weighted in (False, True):
            def call():
                g.hist_reduce_device(K, n_bins, B, 1, d_hist.data_ptr(), d_sums.data_ptr(), 0, windows=windows,
                                     d_weight=d_weight.data_ptr() if weighted else 0, stream=stream)
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            r = dict(what="hare_hist_reduce_device", K=K, n_bins=n_bins, B=B, weights=weighted, n_win=len(windows), n_lev=0, hist_bytes=words * 8,
                     **stats(events_ms(torch, call, a.reps)))
            print(json.dumps(r), flush=True)
            reduce_ms[weighted] = r["median_ms"]
        # yardstick 2: the copy to pinned host memory
        pinned = torch.empty(words, dtype=torch.int64, pin_memory=True)
        pinned.copy_(d_hist)                                                 # first touch
        torch.cuda.synchronize()
        r = dict(what="device-to-host copy, pinned", K=K, n_bins=n_bins, B=B, hist_bytes=words * 8,
                 **stats(events_ms(torch, lambda: pinned.copy_(d_hist, non_blocking=True), a.copy_reps)))
        r["GB_per_s"] = round(words * 8 / (r["median_ms"] * 1e-3) / 1e9, 2)
        print(json.dumps(r), flush=True)
        copy_ms = r["median_ms"]
        del pinned
        for weighted in (False, True):
            t = {}
            for J in vectors:
                def call():
                    g.hist_project_device(K, n_bins, B, 1, d_hist.data_ptr(), J, d_coef.data_ptr(), d_proj.data_ptr(),
                                          d_weight=d_weight.data_ptr() if weighted else 0, stream=stream)
                for _ in range(3):
                    call()
                torch.cuda.synchronize()
                r = dict(what="hare_hist_project_device", K=K, n_bins=n_bins, B=B, J=J, weights=weighted, hist_bytes=words * 8,
                         **stats(events_ms(torch, call, a.reps)))
                r["hbm_fraction"] = round(words * 8 / (r["median_ms"] * 1e-3) / HBM_PEAK, 4)
                r["time_over_reduce"] = round(r["median_ms"] / reduce_ms[weighted], 2)
                r["copy_over_time"] = round(copy_ms / r["median_ms"], 1)
                print(json.dumps(r), flush=True)
                t[J] = r["median_ms"]
            if len(vectors) > 1:
                lo, hi = min(vectors), max(vectors)
                print(json.dumps(dict(what="cost per added vector", K=K, n_bins=n_bins, B=B, weights=weighted,
                                      ms_per_vector=round((t[hi] - t[lo]) / (hi - lo), 5),
                                      steps={f"{p}->{q}": round((t[q] - t[p]) / (q - p), 5) for p, q in zip(sorted(vectors), sorted(vectors)[1:])})), flush=True)
        del d_hist


if __name__ == "__main__":
    main()
