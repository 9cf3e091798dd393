"""Cost of the directional projection (include/hare_hip.h, "receivers", "Directional projection"; kernel hare_hist_project_channels,
project_channels.hip) beside the projection of W alone on the same histogram and beside the memory roofline.  A developer tool; needs an
MI355X and torch.

The shape is tools/bench_project.py's largest map, n_bins = 1 024 and B = 8, with as many receivers as K x n_bins x B x channels <= 2^27
allows: K = 1 820 at nine channels, 1 024 at sixteen (--channels).  A device histogram is filled from a seed (every word random, the
signed channels of either sign) and hare_hist_project_channels_device is timed for J = 8 and 29 vectors (--vectors), without and with
weights: device events around one call, a warm-up first, the median of --reps (default 10) with its range.  The coefficients are the STI
table of hare_amd.sti.mtf_vectors, cut to J rows.  From the same run, beside each figure: hare_hist_project_device on the same histogram
(it fetches the same lines and does 1 / channels of the arithmetic), the ratio of the two, `parent_x_channels` -- what `channels` calls of
the parent on strided views would cost at that rate -- and roofline_ms, the time one read of the histogram per sweep of eight vectors
takes at the 8 TB/s HBM peak.  Neither is a pass mark.  Receiver 0 of a timed result is compared with the integer restatement
(tests/project_channels_ref.py) bit for bit before anything is printed for that shape.

  python tools/bench_project_channels.py [--reps 10] [--channels 9,16] [--vectors 8,29] [--n-bins 1024] [--bands 8]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hare_amd as H  # noqa: E402
from hare_amd import sti  # noqa: E402
from tests.project_channels_ref import project_channels_ref  # noqa: E402

HBM_PEAK = 8.0e12
GROUP = 8                                    # vectors per sweep (hare_amd/csrc/hare_device.h: kProjectGroup)


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--channels", default="9,16")
    ap.add_argument("--vectors", default="8,29")
    ap.add_argument("--n-bins", type=int, default=1024)
    ap.add_argument("--bands", type=int, default=8)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    import torch
    if H.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("bench_project_channels: no GPU -- there is nothing to measure without one")
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    stream = torch.cuda.current_stream().cuda_stream
    vectors = [int(x) for x in a.vectors.split(",")]
    n_bins, B = a.n_bins, a.bands
    weight = H.air_weights(np.linspace(0.001, 0.02, B), 0.01, n_bins)
    d_weight = torch.from_numpy(weight.view(np.int32)).to("cuda")
    table = sti.mtf_vectors(n_bins, 0.01, 1.0)                               # 29 x n_bins: 10 ms bins
    d_coef = torch.from_numpy(table).to("cuda")
    for C in (int(x) for x in a.channels.split(",")):
        K = min(65536, (1 << 27) // (n_bins * B * C))
        words = K * n_bins * B * C
        gen = torch.Generator(device="cuda").manual_seed(7)
        d_hist = torch.randint(-(1 << 63), (1 << 63) - 1, (words,), dtype=torch.int64, device="cuda", generator=gen)
        d_proj = torch.zeros(K * B * max(vectors) * C * 2, dtype=torch.int64, device="cuda")
        d_parent = torch.zeros(K * B * max(vectors) * 2, dtype=torch.int64, device="cuda")
        first = d_hist[:n_bins * B * C].cpu().numpy().view(np.uint64).reshape(1, n_bins, B, C)
        for weighted in (False, True):
            w_ptr = d_weight.data_ptr() if weighted else 0
            for J in vectors:
                def call():
                    g.hist_project_channels_device(K, n_bins, B, C, d_hist.data_ptr(), J, d_coef.data_ptr(), d_proj.data_ptr(), d_weight=w_ptr, stream=stream)

                def parent():
                    g.hist_project_device(K, n_bins, B, C, d_hist.data_ptr(), J, d_coef.data_ptr(), d_parent.data_ptr(), d_weight=w_ptr, stream=stream)
                for _ in range(3):
                    call()
                    parent()
                torch.cuda.synchronize()
                t_new = stats(events_ms(torch, call, a.reps))
                t_par = stats(events_ms(torch, parent, a.reps))
                # a window of the timed result against the restatement: receiver 0, every band, vector and channel
                got = d_proj[:B * J * C * 2].cpu().numpy().view(np.uint64).reshape(1, B, J, C, 2)
                if got.tobytes() != project_channels_ref(first, table[:J], weight if weighted else None).tobytes():
                    raise SystemExit("bench_project_channels: receiver 0 differs from the restatement")
                sweeps = (J + GROUP - 1) // GROUP
                r = dict(what="hare_hist_project_channels_device", K=K, n_bins=n_bins, B=B, channels=C, J=J, weights=weighted, hist_bytes=words * 8,
                         **t_new, parent_median_ms=t_par["median_ms"], parent_min_ms=t_par["min_ms"], parent_max_ms=t_par["max_ms"])
                r["time_over_parent"] = round(t_new["median_ms"] / t_par["median_ms"], 2)
                r["parent_x_channels_ms"] = round(t_par["median_ms"] * C, 3)
                r["sweeps"] = sweeps
                r["roofline_ms"] = round(sweeps * words * 8 / HBM_PEAK * 1e3, 4)
                r["time_over_roofline"] = round(t_new["median_ms"] / r["roofline_ms"], 2)
                print(json.dumps(r), flush=True)
        del d_hist, d_proj, d_parent


if __name__ == "__main__":
    main()
