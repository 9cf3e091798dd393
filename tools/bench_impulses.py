"""Cost of turning a per-sample histogram into pressure rows (include/hare_hip.h, "receivers", "Impulses"; kernel hare_hist_impulses,
impulses.hip), after tools/bench_decode.py.  A developer tool; needs an MI355X and torch.

Three timings in one run, each with device events around the calls of ONE job, a warm-up first, the median of --reps jobs and their range:

  sparse         the shape of an early part: K = 256 receivers at third order (16 channels), n_bins = 4800 (100 ms at 48 kHz), B = 8 bands,
                 T = 511 taps, and --entries (200) entries per receiver and band at seeded bins; the whole output, n_bins + T - 1 samples.
                 K x n_bins x B x channels is above the 2^27 words one call takes, so the job is cut over the receivers into the fewest
                 calls that fit -- by the definition the one call byte for byte -- and the calls are timed together
  dense          the same shape with every bin an entry: what the sparse kernel costs when nothing is sparse
  decode         the baseline from before this kernel: the dense formulation through hare_decode_device at K x channels receivers,
                 C = B, O = 1, N = n_bins, the same T, on arbitrary finite data.  A figure to compare against, not one to beat when dense

Receiver 0 of each impulse result is compared bit for bit with the numpy restatement (tests/impulse_ref.py); a window of the decode's with
tests/decode_ref.py.  entries_per_s is entries over the median time; terms are entries x channels x T (every entry meets T outputs).

  python tools/bench_impulses.py [--reps 20] [--shape 256x4800x8x16x511] [--entries 200]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hare_amd as H  # noqa: E402
from tests.decode_ref import decode_ref  # noqa: E402
from tests.impulse_ref import impulse_ref  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shape", default="256x4800x8x16x511", help="K x n_bins x B x channels x T")
    ap.add_argument("--entries", type=int, default=200, help="entries per receiver and band of the sparse histogram")
    a = ap.parse_args()
    import torch
    if H.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("bench_impulses: no GPU -- there is nothing to measure without one")
    K, nb, B, C, T = (int(v) for v in a.shape.split("x"))
    frac_bits, n_out = 24, nb + T - 1
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    rng = np.random.default_rng(2026)
    torch.manual_seed(2026)
    stream = torch.cuda.current_stream().cuda_stream
    taps = rng.standard_normal((B, T))
    d_taps = torch.from_numpy(taps).to("cuda")
    d_out = torch.zeros((K, C, n_out), dtype=torch.float64, device="cuda")
    per_call = max(1, min(K, (1 << 27) // (nb * B * C)))
    cuts = list(range(0, K, per_call)) + [K]

    def words(shape):
        """random histogram words on the device: W in [1, 2^40), the signed channels within +-W"""
        W = torch.randint(1, 1 << 40, shape, dtype=torch.int64, device="cuda")
        sub = ((torch.rand(shape + (C - 1,), dtype=torch.float64, device="cuda") * 2 - 1) * W[..., None].to(torch.float64)).to(torch.int64)
        return torch.cat([W[..., None], sub], dim=-1)

    def job(d_hist):
        for k0, k1 in zip(cuts, cuts[1:]):
            g.hist_impulses_device(k1 - k0, nb, B, C, d_hist[k0].data_ptr(), frac_bits, T, d_taps.data_ptr(), 0, n_out, n_out, 0, d_out[k0].data_ptr(),
                                   stream=stream)

    def impulse_run(d_hist, entries):
        med, lo, hi = timed(lambda: job(d_hist), a.reps)
        hist0 = d_hist[0].cpu().numpy().view(np.uint64)[None]
        ok = same_bits(d_out[0].cpu().numpy()[None], impulse_ref(hist0, taps, frac_bits)) is None
        return dict(K=K, n_bins=nb, B=B, channels=C, T=T, n_out=n_out, calls=len(cuts) - 1, entries=entries, median_ms=round(med, 3), min_ms=round(lo, 3),
                    max_ms=round(hi, 3), n=a.reps, entries_per_s=round(entries / (med * 1e-3)), terms=entries * C * T,
                    terms_per_s=round(entries * C * T / (med * 1e-3), -8), receiver_0_matches_reference=ok)

    # sparse: --entries bins per (receiver, band), drawn without repetition
    d_hist = torch.zeros((K, nb, B, C), dtype=torch.int64, device="cuda")
    at = np.argsort(rng.random((K, B, nb)), axis=2)[:, :, :a.entries]                           # [K, B, entries] bins
    kk, bb = np.meshgrid(np.arange(K), np.arange(B), indexing="ij")
    idx = (torch.from_numpy(np.repeat(kk[..., None], a.entries, 2).reshape(-1)).to("cuda"), torch.from_numpy(at.reshape(-1)).to("cuda"),
           torch.from_numpy(np.repeat(bb[..., None], a.entries, 2).reshape(-1)).to("cuda"))
    d_hist[idx] = words((K * B * a.entries,))
    sparse_row = impulse_run(d_hist, K * B * a.entries)
    # dense: every bin an entry
    d_hist.copy_(words((K, nb, B)))
    dense_row = impulse_run(d_hist, K * B * nb)
    del d_hist
    torch.cuda.empty_cache()

    # the baseline: the dense formulation through the decode kernel
    R = K * C
    x, h = torch.randn((R, B, nb), dtype=torch.float64, device="cuda"), torch.randn((1, B, T), dtype=torch.float64, device="cuda")
    d_y = torch.zeros((R, 1, n_out), dtype=torch.float64, device="cuda")
    med, lo, hi = timed(lambda: g.decode_device(R, B, nb, x.data_ptr(), 1, T, h.data_ptr(), 0, n_out, d_y.data_ptr(), stream=stream), a.reps)
    w0 = n_out // 2
    ok = same_bits(d_y[:2, :, w0:w0 + 64].cpu().numpy(), decode_ref(x[:2].cpu().numpy(), h.cpu().numpy(), w0, 64)) is None
    decode_row = dict(K=R, C=B, N=nb, O=1, T=T, n_out=n_out, median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), n=a.reps,
                      terms=R * B * nb * T, terms_per_s=round(R * B * nb * T / (med * 1e-3), -8), window_matches_reference=ok)
    print(json.dumps(dict(what="hare_hist_impulses_device", sparse=sparse_row, dense=dense_row, decode=decode_row,
                          sparse_over_decode=round(sparse_row["median_ms"] / decode_row["median_ms"], 4),
                          dense_over_decode=round(dense_row["median_ms"] / decode_row["median_ms"], 4))), flush=True)


if __name__ == "__main__":
    main()
