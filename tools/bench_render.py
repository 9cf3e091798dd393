"""Cost of rendering a histogram to impulse responses (include/hare_hip.h, "receivers", "Rendering"; kernel hare_hist_render, render.hip).
A developer tool; needs an MI355X and torch.

The shape (default K = 256, n_bins = 400, M = 240, B = 8, T = 511, channels = 16: 256 third-order receivers, 2 s at 48 kHz in 5 ms bins,
octave bands) is filled from a seed and rendered with band_taps filters.  hare_hist_render_device refuses more than 2^28 output samples in
one call, and this shape has 1.46 times that, so the receivers go in as few equal calls as fit (two of K = 128 here), back to back on one
stream into one output buffer; device events surround the calls of one repetition, a warm-up comes first, and the median of --reps
repetitions and their spread are printed.  Beside it: the FP64 additions the definition needs, counted from the shape -- K B N T for y (an
fma each on the device), K B N for p, K channels N (B - 1) for the output --, their rate, and that rate as a fraction of the vector FP64 peak.
MI355X_MICROARCH.md lists the vector FP32 peak only (157.3 TFLOPS, 64 FLOP per clock and SIMD); the vector FP64 rate of the part is half
of it, 78.6 TFLOPS counting an fma as two, that is 39.3e12 additions (or fmas) per second, and that is the peak used here.  Receiver 0 of
the result is compared bit for bit with the numpy restatement (tests/render_ref.py), whose time on that one receiver is printed for scale.

  python tools/bench_render.py [--reps 50] [--shape 256x400x240x8x511x16]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hare_amd as H  # noqa: E402
from tests.receive_harness import same_bits  # noqa: E402
from tests.render_ref import render_ref  # noqa: E402

FP64_ADDS_PER_S = 39.3e12          # 256 CUs x 4 SIMDs x 16 FP64 lanes x 2.4 GHz
MAX_OUT = 1 << 28


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--shape", default="256x400x240x8x511x16", help="K x n_bins x M x B x T x channels")
    a = ap.parse_args()
    import torch
    if H.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("bench_render: no GPU -- there is nothing to measure without one")
    K, n_bins, M, B, T, C = (int(x) for x in a.shape.split("x"))
    N, frac_bits, seed = n_bins * M, 30, 2024
    calls = -(-K * C * N // MAX_OUT)
    while K % calls:
        calls += 1
    Kc = K // calls
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    taps = H.band_taps(48000.0, [88.0 * 2 ** b for b in range(B - 1)], T) if B > 1 else np.ones((1, T)) / T
    rng = np.random.default_rng(11)
    decay = 2.0 ** (40 - 20 * np.arange(n_bins) / n_bins)[None, :, None]            # 60 dB over the histogram
    W = np.floor(decay * rng.uniform(0.5, 1.5, (K, n_bins, B))).astype(np.uint64)
    hist = np.zeros((K, n_bins, B, C), np.uint64)
    hist[..., 0] = W
    if C > 1:
        hist[..., 1:] = np.trunc(rng.uniform(-1, 1, (K, n_bins, B, C - 1)) * W[..., None].astype(np.float64)).astype(np.int64).view(np.uint64)
    d_hist = torch.from_numpy(hist.view(np.int64)).to("cuda")
    d_taps = torch.from_numpy(taps).to("cuda")
    d_out = torch.zeros(Kc * C * N, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    words = Kc * n_bins * B * C

    def rep(only=None):
        for c in range(calls) if only is None else [only]:
            g.hist_render_device(Kc, n_bins, B, C, d_hist.data_ptr() + 8 * words * c, frac_bits, M, T, d_taps.data_ptr(), seed, d_out.data_ptr(),
                                 stream=stream)

    rep()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rep()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    rep(only=0)                                                                      # the first call's receivers: k = 0 is the reference's
    torch.cuda.synchronize()
    first = d_out[:C * N].cpu().numpy().reshape(1, C, N)
    t0 = time.perf_counter()
    want = render_ref(hist[:1], taps, M, frac_bits, seed)
    ref_s = time.perf_counter() - t0
    adds = K * B * N * T + K * B * N + K * C * N * (B - 1)
    med = statistics.median(ms)
    print(json.dumps(dict(what="hare_hist_render_device", K=K, n_bins=n_bins, M=M, B=B, T=T, channels=C, calls=calls, K_per_call=Kc,
                          median_ms=round(med, 2), min_ms=round(min(ms), 2), max_ms=round(max(ms), 2), n=len(ms), fp64_adds=adds,
                          adds_per_s=round(adds / (med * 1e-3), -9), fraction_of_fp64_vector_peak=round(adds / (med * 1e-3) / FP64_ADDS_PER_S, 4),
                          out_bytes=K * C * N * 8, numpy_reference_one_receiver_s=round(ref_s, 2),
                          receiver_0_matches_reference=same_bits(first, want) is None)), flush=True)


if __name__ == "__main__":
    main()
