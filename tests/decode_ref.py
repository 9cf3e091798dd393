"""The numpy restatement of hare_decode (include/hare_hip.h, "receivers", "Decoding"): K x C rows of N doubles decoded to K x O rows through
O x C FIR filters of T doubles, a window [n0, n0 + n_out) of the N + T - 1 samples.  The header's order and nothing else:

    t_lo = max(0, n - (N - 1));   t_hi = min(T - 1, n)
    acc = +0.0
    for c ascending:   for t = t_lo .. t_hi ascending:   acc = acc + h[o, c, t] * in[k, c, n - t]

A loop over c, then t, vectorised over (k, o, n).  For one t the outputs whose range holds it are the contiguous run t <= n <= t + N - 1,
and only those are touched: a term out of range is skipped, never formed against a zero.  numpy rounds the product, then the add (two
ufuncs, no fused multiply-add).  A NaN result is "some NaN": compare through tests/convolve_ref.py's `canonical` (or
tests/receive_harness.py: same_bits).  No GPU, no torch."""
import numpy as np

ORDERS = ("definition", "c descending", "t outer", "per channel")


def decode_ref(in_, h, n0=0, n_out=None, order="definition"):
    """float64 [K, O, n_out].  in_: [K, C, N]; h: [O, C, T].  order: "definition", or one of three MUTANTS that are not the definition and
    that tests/test_decode_cases.py uses to show that the cases can see a wrong order -- "c descending" (the channels from C - 1 down),
    "t outer" (for t: for c), "per channel" (every channel's convolution summed from +0.0 on its own, the C results added in ascending c
    afterwards: what hare_convolve per channel and an add on the host would give)."""
    in_, h = np.ascontiguousarray(in_, np.float64), np.ascontiguousarray(h, np.float64)
    assert in_.ndim == 3 and h.ndim == 3 and in_.shape[1] == h.shape[1] and order in ORDERS
    (K, C, N), (O, _, T) = in_.shape, h.shape
    n0 = int(n0)
    n_out = N + T - 1 - n0 if n_out is None else int(n_out)
    assert N >= 1 and T >= 1 and n0 >= 0 and n_out >= 1 and n0 + n_out <= N + T - 1
    taps = range(max(0, n0 - (N - 1)), min(T - 1, n0 + n_out - 1) + 1)      # the taps any output of the window meets
    chans = range(C - 1, -1, -1) if order == "c descending" else range(C)
    terms = [(c, t) for t in taps for c in chans] if order == "t outer" else [(c, t) for c in chans for t in taps]
    acc = np.zeros((K, O, n_out), np.float64)                                # +0.0
    part = np.zeros((C, K, O, n_out), np.float64) if order == "per channel" else None
    with np.errstate(all="ignore"):
        for c, t in terms:
            a, b = max(t, n0), min(t + N - 1, n0 + n_out - 1)               # the outputs n with 0 <= n - t <= N - 1, inside the window
            if a > b:
                continue
            run = (acc if part is None else part[c])[:, :, a - n0:b - n0 + 1]
            run += h[None, :, c, t:t + 1] * in_[:, None, c, a - t:b - t + 1]          # the rounded product, then the add
        if part is not None:
            for c in chans:
                acc += part[c]
    return acc
