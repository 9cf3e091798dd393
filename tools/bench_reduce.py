"""Cost of the histogram reduction (include/hare_hip.h, "receivers", "Reduction"; kernel hare_hist_reduce, reduce.hip) beside the copy it
replaces.  A developer tool; needs an MI355X and torch.

For each shape (default: K = 16 384, n_bins = 1 024, B = 8 -- the 1 GiB cap -- and K = 1 024, n_bins = 4 000, B = 8) a device histogram
is filled from a seed, flat (uniform words: the -35 dB crossing lies in the last bins, so pass 2 runs to the end -- the worst case) or as
a decay of 60 dB over the histogram (pass 2 ends early), and hare_hist_reduce_device is timed with 4 windows and the 31 levels -5 .. -35
dB, without and with weights: device events around one call, a warm-up first, the median of --reps (default 25, at least 20) and the
spread.  In the same run the device-to-host copy of the same histogram is timed, into pinned and into pageable host memory (events and a
synchronise; median of --copy-reps).  Printed, one JSON object per line: the times in ms; hbm_fraction, the histogram's bytes COUNTED ONCE
over the kernel's time as a fraction of the 8 TB/s HBM peak (the kernel reads the block again in pass 2, and once more per four windows
beyond the first four: those reads are expected from L2 and are not counted, so this is the share of the one compulsory read, not the
kernel's traffic); and for each copy its ratio to each of the four kernel times (flat / decay, without / with weights).

  python tools/bench_reduce.py [--reps 25] [--copy-reps 7] [--shapes 16384x1024x8,1024x4000x8]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hare_amd as H  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--copy-reps", type=int, default=7)
    ap.add_argument("--shapes", default="16384x1024x8,1024x4000x8")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    if H.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("bench_reduce: no GPU -- there is nothing to measure without one")
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    levels = H.decay_levels(-np.arange(5.0, 36.0))
    stream = torch.cuda.current_stream().cuda_stream
    for shape in a.shapes.split(","):
        K, n_bins, B = (int(x) for x in shape.split("x"))
        words = K * n_bins * B
        windows = [(0, n_bins), (0, n_bins // 20), (0, n_bins // 12), (n_bins // 12, n_bins)]
        gen = torch.Generator(device="cuda").manual_seed(7)
        d_hist = torch.randint(0, 1 << 40, (words,), dtype=torch.int64, device="cuda", generator=gen)
        d_weight = torch.from_numpy(H.air_weights(np.linspace(0.001, 0.02, B), 0.01, n_bins).view(np.int32)).to("cuda")
        d_sums = torch.zeros(K * B * len(windows) * 4, dtype=torch.int64, device="cuda")
        d_cross = torch.zeros(K * B * len(levels), dtype=torch.int32, device="cuda")
        kernel_ms = {}
        for fill in ("flat", "decay"):
            if fill == "decay":                      # 60 dB over the histogram: a shift of 20 bits
                shift = (torch.arange(n_bins, device="cuda", dtype=torch.int64) * 20 // n_bins).view(1, n_bins, 1)
                d_hist = (d_hist.view(K, n_bins, B) >> shift).reshape(-1).contiguous()
            for weighted in (False, True):
                def call():
                    g.hist_reduce_device(K, n_bins, B, 1, d_hist.data_ptr(), d_sums.data_ptr(), d_cross.data_ptr(), windows=windows, levels=levels,
                                         d_weight=d_weight.data_ptr() if weighted else 0, stream=stream)
                for _ in range(3):
                    call()
                torch.cuda.synchronize()
                ms = events_ms(torch, call, a.reps)
                r = dict(what="hare_hist_reduce_device", K=K, n_bins=n_bins, B=B, fill=fill, weights=weighted, n_win=len(windows), n_lev=len(levels),
                         hist_bytes=words * 8, **stats(ms))
                r["hbm_fraction"] = round(words * 8 / (r["median_ms"] * 1e-3) / HBM_PEAK, 4)
                r["last_crossing_max"] = int(d_cross.max().item())
                print(json.dumps(r), flush=True)
                kernel_ms[fill + (", weights" if weighted else ", no weights")] = r["median_ms"]
        pinned = torch.empty(words, dtype=torch.int64, pin_memory=True)
        pageable = torch.empty(words, dtype=torch.int64)
        for name, host in (("pinned", pinned), ("pageable", pageable)):
            host.copy_(d_hist)                       # first touch
            torch.cuda.synchronize()
            if name == "pinned":
                ms = events_ms(torch, lambda: host.copy_(d_hist, non_blocking=True), a.copy_reps)
            else:
                ms = []
                for _ in range(a.copy_reps):
                    t0 = time.perf_counter()
                    host.copy_(d_hist)
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3)
            r = dict(what="device-to-host copy, " + name, K=K, n_bins=n_bins, B=B, hist_bytes=words * 8, **stats(ms))
            r["GB_per_s"] = round(words * 8 / (r["median_ms"] * 1e-3) / 1e9, 2)
            r["ratio_to_kernel"] = {k: round(r["median_ms"] / v, 1) for k, v in kernel_ms.items()}
            print(json.dumps(r), flush=True)
        del d_hist, pinned, pageable


if __name__ == "__main__":
    main()
