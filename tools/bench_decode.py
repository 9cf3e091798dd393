"""Cost of decoding rendered responses through a matrix of FIR filters (include/hare_hip.h, "receivers", "Decoding"; kernel hare_decode,
decode.hip), after tools/bench_convolve.py.  A developer tool; needs an MI355X and torch.

Three timings in one run, each with device events around ONE call, a warm-up first, the median of --reps calls and their range:

  decode         the main shape (default K = 16 receivers at third order, C = 16, N = 96 000, two seconds at 48 kHz, decoded to O = 2 ears
                 through filters of T = 512 taps, the whole output), standard normals from a seed.  A window of 64 outputs of every row of
                 the timed result is compared bit for bit with the numpy restatement (tests/decode_ref.py)
                 burst_ms_per_call: --burst calls back to back between one pair of events, per call -- a single call of a few milliseconds
                 behind a synchronisation is timed while the clock is still rising, a window of a few hundred is not
  convolve       the yardstick: hare_convolve_device on its own bench shape (R = 16, N = 96 000, L = 480 000), the same instruction mix
  matrix         the edge path: a plain gain matrix, T = 1 with C = 16 and O = 8 on the same K and N.  Stated, not specialised

and beside them:

  terms          K x O x C x N x T, the multiply-add pairs the definition needs (every product of a tap and a sample appears in exactly one output)
  terms_per_s    terms over the median time; ratio_to_convolve is the decode's over the yardstick's
  fraction       of the chip's vector FP64 rate as DESIGN.md 7b ("Convolution") derives it: CUs x 4 SIMDs x 16 lanes x clock instructions
                 per second, CUs and clock as the device reports them, two instructions to a term
  cap            the largest power of two of terms that one launch finishes in under two seconds at the measured rate, the figure behind
                 HARE_DECODE_MAX_TERMS.  The call bounds K x O x n_out x C x min(N, T), which is never less than the terms

  python tools/bench_decode.py [--reps 10] [--shape 16x16x96000x2x512] [--matrix 16x16x96000x8x1] [--convolve 16x96000x480000]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hare_amd as H  # noqa: E402
from tests.decode_ref import decode_ref  # noqa: E402
from tests.receive_harness import same_bits  # noqa: E402


def timed(call, reps):
    """(median, min, max) in ms of `reps` calls, device events around each, one warm-up first"""
    import torch
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def burst(call, n):
    """ms per call of n calls back to back between ONE pair of events: a window long enough that the clock has settled"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--burst", type=int, default=64, help="calls back to back in one timed window, beside the single calls")
    ap.add_argument("--shape", default="16x16x96000x2x512", help="K x C x N x O x T")
    ap.add_argument("--matrix", default="16x16x96000x8x1", help="K x C x N x O x T of the edge-path matrix")
    ap.add_argument("--convolve", default="16x96000x480000", help="R x N x L of the yardstick")
    a = ap.parse_args()
    import torch
    if H.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("bench_decode: no GPU -- there is nothing to measure without one")
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    rng = np.random.default_rng(2026)
    stream = torch.cuda.current_stream().cuda_stream
    hip = ctypes.CDLL(H.capi.lib.hare_hip_runtime_path().decode())          # the runtime the library bound
    khz = ctypes.c_int(0)
    if hip.hipDeviceGetAttribute(ctypes.byref(khz), 5, 0) != 0 or khz.value <= 0:          # hipDeviceAttributeClockRate, kHz
        raise SystemExit("bench_decode: the device does not report its clock")
    cus, clock_hz = torch.cuda.get_device_properties(0).multi_processor_count, khz.value * 1e3
    peak_terms = cus * 4 * 16 * clock_hz / 2

    def decode_run(shape, check):
        K, C, N, O, T = (int(v) for v in shape.split("x"))
        n_out = N + T - 1
        x, h = rng.standard_normal((K, C, N)), rng.standard_normal((O, C, T))
        d_x, d_h = torch.from_numpy(x).to("cuda"), torch.from_numpy(h).to("cuda")
        d_y = torch.zeros(K * O * n_out, dtype=torch.float64, device="cuda")
        call = lambda: g.decode_device(K, C, N, d_x.data_ptr(), O, T, d_h.data_ptr(), 0, n_out, d_y.data_ptr(), stream=stream)  # noqa: E731
        med, lo, hi = timed(call, a.reps)
        terms = K * O * C * N * T
        row = dict(K=K, C=C, N=N, O=O, T=T, n_out=n_out, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), n=a.reps, terms=terms,
                   terms_per_s=round(terms / (med * 1e-3), -8), burst_calls=a.burst, burst_ms_per_call=round(burst(call, a.burst), 3))
        if check:
            y = d_y.cpu().numpy().reshape(K, O, n_out)
            w0 = n_out // 2
            row["window_matches_reference"] = same_bits(y[:, :, w0:w0 + 64], decode_ref(x, h, w0, 64)) is None
        return row

    main_row = decode_run(a.shape, True)
    matrix_row = decode_run(a.matrix, True)

    R, N, L = (int(v) for v in a.convolve.split("x"))
    d_ir, d_s = torch.from_numpy(rng.standard_normal((R, N))).to("cuda"), torch.from_numpy(rng.standard_normal(L)).to("cuda")
    d_c = torch.zeros(R * (N + L - 1), dtype=torch.float64, device="cuda")
    med, lo, hi = timed(lambda: g.convolve_device(R, N, d_ir.data_ptr(), L, d_s.data_ptr(), 0, N + L - 1, d_c.data_ptr(), stream=stream), a.reps)
    conv_row = dict(R=R, N=N, L=L, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), n=a.reps, terms=R * N * L,
                    terms_per_s=round(R * N * L / (med * 1e-3), -8))

    rate = main_row["terms"] / (main_row["median_ms"] * 1e-3)
    cap = 1
    while 2 * cap / rate < 2.0:
        cap *= 2
    print(json.dumps(dict(what="hare_decode_device", decode=main_row, convolve=conv_row, matrix=matrix_row, cus=cus, clock_mhz=round(clock_hz / 1e6),
                          peak_terms_per_s=round(peak_terms, -9), fraction_of_fp64_vector_peak=round(rate / peak_terms, 4),
                          ratio_to_convolve=round(rate / (conv_row["terms"] / (conv_row["median_ms"] * 1e-3)), 4),
                          matrix_fraction_of_fp64_vector_peak=round(matrix_row["terms"] / (matrix_row["median_ms"] * 1e-3) / peak_terms, 4),
                          cap_log2=cap.bit_length() - 1, seconds_at_cap=round(cap / rate, 3))), flush=True)


if __name__ == "__main__":
    main()
