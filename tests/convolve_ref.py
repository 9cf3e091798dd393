"""The numpy restatement of hare_convolve (include/hare_hip.h, "receivers", "Convolution"): R rows of N doubles, each convolved in the time
domain with one signal of L doubles, a window [n0, n0 + n_out) of the full convolution.  The header's order and nothing else:

    t_lo = max(0, n - (L - 1));   t_hi = min(N - 1, n)
    acc = +0.0;   for t = t_lo .. t_hi ascending:   acc = acc + ir[r, t] * x[n - t]

A loop over t, vectorised over (r, n).  For one t the outputs whose range holds it are the contiguous run t <= n <= t + L - 1, and only
those are touched: a term out of range is skipped, never formed against a zero.  numpy rounds the product, then the add (two ufuncs, no
fused multiply-add).  A NaN result is "some NaN": compare through `canonical` (or tests/receive_harness.py: same_bits).  No GPU, no torch."""
import numpy as np


def convolve_ref(ir, x, n0=0, n_out=None, descending=False):
    """float64 [R, n_out].  ir: [R, N] (or [K, C, N], flattened to rows k * C + ch); x: [L].  descending: the MUTANT that walks t from
    t_hi down to t_lo -- not the definition; tests/test_convolve_cases.py uses it to show that the cases can see a wrong order."""
    ir, x = np.ascontiguousarray(ir, np.float64), np.ascontiguousarray(x, np.float64)
    ir = ir.reshape(-1, ir.shape[-1])
    (R, N), L = ir.shape, x.shape[0]
    n0 = int(n0)
    n_out = N + L - 1 - n0 if n_out is None else int(n_out)
    assert N >= 1 and L >= 1 and n0 >= 0 and n_out >= 1 and n0 + n_out <= N + L - 1
    acc = np.zeros((R, n_out), np.float64)                                   # +0.0
    taps = range(max(0, n0 - (L - 1)), min(N - 1, n0 + n_out - 1) + 1)      # the taps any output of the window meets
    with np.errstate(all="ignore"):
        for t in (reversed(taps) if descending else taps):
            a, b = max(t, n0), min(t + L - 1, n0 + n_out - 1)               # the outputs n with 0 <= n - t <= L - 1, inside the window
            if a > b:
                continue
            part = acc[:, a - n0:b - n0 + 1]
            part += ir[:, t:t + 1] * x[None, a - t:b - t + 1]               # the rounded product, then the add
    return acc


def canonical(y):
    """y with every NaN replaced by the one quiet NaN 0x7FF8000000000000: what is left is defined to the bit."""
    y = np.array(y, np.float64)
    y[np.isnan(y)] = np.float64(np.nan)
    w = y.view(np.uint64)
    w[np.isnan(y)] = np.uint64(0x7FF8000000000000)
    return y
