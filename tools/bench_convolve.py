"""Cost of convolving rendered responses with a dry signal (include/hare_hip.h, "receivers", "Convolution"; kernel hare_convolve,
convolve.hip).  A developer tool; needs an MI355X and torch.

The shape (default R = 16, N = 96 000, L = 480 000: one third-order receiver of two seconds against ten seconds of signal at 48 kHz, the
whole output) is filled with standard normals from a seed.  Device events surround ONE hare_convolve_device call; a warm-up comes first,
and the median of --reps calls and their spread are printed.  Beside it:

  terms          R x N x L, the multiply-add pairs the definition needs (every product of a tap and a sample appears in exactly one output)
  terms_per_s    terms over the median time
  fraction       of the chip's vector FP64 rate.  A SIMD issues one FP64 instruction to 16 lanes per clock, so the chip does
                 CUs x 4 SIMDs x 16 lanes x clock instructions per second, CUs and clock as the device reports them (torch's multi_processor_count;
                 hipDeviceAttributeClockRate, asked of the runtime the library bound); a term is TWO instructions here, a multiply and an add, because the definition forbids the fused one: the
                 peak in terms is half of that.  The clock is the reported maximum; the chip runs below it under load
  cap            the largest power of two of terms that one launch finishes in under two seconds at the measured rate, the figure behind
                 HARE_CONVOLVE_MAX_TERMS.  The call bounds R x n_out x min(N, L), which is never less than the terms
  host           the same job with scipy.signal.fftconvolve per row (np.convolve where scipy is absent), as context, not as a pass mark: an
                 FFT takes far fewer operations and has no stated order of its sums

A window of 64 outputs of every row is compared bit for bit with the numpy restatement (tests/convolve_ref.py).

  python tools/bench_convolve.py [--reps 10] [--shape 16x96000x480000]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hare_amd as H  # noqa: E402
from tests.convolve_ref import convolve_ref  # noqa: E402
from tests.receive_harness import same_bits  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape", default="16x96000x480000", help="R x N x L")
    a = ap.parse_args()
    import torch
    if H.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("bench_convolve: no GPU -- there is nothing to measure without one")
    R, N, L = (int(v) for v in a.shape.split("x"))
    n_out = N + L - 1
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    rng = np.random.default_rng(2025)
    ir, x = rng.standard_normal((R, N)), rng.standard_normal(L)
    d_ir, d_x = torch.from_numpy(ir).to("cuda"), torch.from_numpy(x).to("cuda")
    d_y = torch.zeros(R * n_out, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        g.convolve_device(R, N, d_ir.data_ptr(), L, d_x.data_ptr(), 0, n_out, d_y.data_ptr(), stream=stream)

    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    y = d_y.cpu().numpy().reshape(R, n_out)
    w0 = n_out // 2
    matches = same_bits(y[:, w0:w0 + 64], convolve_ref(ir, x, w0, 64)) is None
    t0 = time.perf_counter()
    try:
        from scipy.signal import fftconvolve
        host, host_y = "scipy.signal.fftconvolve per row", np.stack([fftconvolve(row, x) for row in ir])
    except ImportError:
        host, host_y = "np.convolve per row", np.stack([np.convolve(row, x) for row in ir])
    host_s = time.perf_counter() - t0
    import ctypes
    hip = ctypes.CDLL(H.capi.lib.hare_hip_runtime_path().decode())          # the runtime the library bound
    khz = ctypes.c_int(0)
    if hip.hipDeviceGetAttribute(ctypes.byref(khz), 5, 0) != 0 or khz.value <= 0:          # hipDeviceAttributeClockRate, kHz
        raise SystemExit("bench_convolve: the device does not report its clock")
    cus, clock_hz = torch.cuda.get_device_properties(0).multi_processor_count, khz.value * 1e3
    peak_terms = cus * 4 * 16 * clock_hz / 2
    terms = R * N * L
    med = statistics.median(ms)
    rate = terms / (med * 1e-3)
    cap = 1
    while 2 * cap / rate < 2.0:
        cap *= 2
    print(json.dumps(dict(what="hare_convolve_device", R=R, N=N, L=L, n_out=n_out, median_ms=round(med, 2), min_ms=round(min(ms), 2),
                          max_ms=round(max(ms), 2), n=len(ms), terms=terms, terms_per_s=round(rate, -9), cus=cus, clock_mhz=round(clock_hz / 1e6),
                          peak_terms_per_s=round(peak_terms, -9), fraction_of_fp64_vector_peak=round(rate / peak_terms, 4),
                          cap_log2=cap.bit_length() - 1, seconds_at_cap=round(cap / rate, 3), host=host, host_s=round(host_s, 2),
                          host_max_abs_difference=float(np.abs(host_y - y).max()), window_matches_reference=matches)), flush=True)


if __name__ == "__main__":
    main()
