"""The reduction of a receive histogram (include/hare_hip.h, "receivers", "Reduction"), restated in Python integers: what hare_hist_reduce
must return, bit for bit.  No floats anywhere.  reduce_direct is the definition word for word (small inputs); reduce_ref the same through
running sums, for the sizes the device tests use (tests/test_hist_reduce_api.py holds the two against each other)."""
from itertools import accumulate

import numpy as np

M64 = (1 << 64) - 1


def _inputs(hist, windows, levels, weight):
    hist = np.asarray(hist, np.uint64)
    if hist.ndim == 4:
        hist = hist[..., 0]                      # channel 0, W
    w = None if weight is None else np.asarray(weight, np.uint32).tolist()
    return hist.shape, hist.tolist(), [(int(lo), int(hi)) for lo, hi in windows], [int(f) for f in levels], w


def _words(x):
    return [x & M64, x >> 64]


def reduce_direct(hist, windows=(), levels=(), weight=None):
    """The definition as the header states it.  hist: uint64 [K, n_bins, B] or [K, n_bins, B, C] (C = 4, 9 or 16: channel 0 is read); windows: (lo, hi) bin pairs; levels:
    uint32 fractions in units of 2^-32; weight: uint32 [n_bins, B] or None.  Returns (sums uint64 [K, B, n_win, 4], cross int32
    [K, B, n_lev])."""
    (K, n_bins, B), h, windows, levels, w = _inputs(hist, windows, levels, weight)
    sums = np.zeros((K, B, len(windows), 4), np.uint64)
    cross = np.zeros((K, B, len(levels)), np.int32)
    for k in range(K):
        for b in range(B):
            g = [h[k][i][b] if w is None else (h[k][i][b] * w[i][b]) >> 32 for i in range(n_bins)]
            for j, (lo, hi) in enumerate(windows):
                sums[k, b, j] = _words(sum(g[lo:hi])) + _words(sum(i * g[i] for i in range(lo, hi)))
            T = sum(g)
            for l, f in enumerate(levels):
                cross[k, b, l] = min(i for i in range(n_bins + 1) if (T - sum(g[:i])) << 32 <= T * f)
    return sums, cross


def reduce_ref(hist, windows=(), levels=(), weight=None):
    """reduce_direct with P(i) and the running sum of i * g kept in lists: a window's sum is a difference of two entries, and a crossing is
    found by bisection on the header's own comparison (R does not increase with i)."""
    (K, n_bins, B), h, windows, levels, w = _inputs(hist, windows, levels, weight)
    sums = np.zeros((K, B, len(windows), 4), np.uint64)
    cross = np.zeros((K, B, len(levels)), np.int32)
    for k in range(K):
        for b in range(B):
            g = [h[k][i][b] if w is None else (h[k][i][b] * w[i][b]) >> 32 for i in range(n_bins)]
            P = [0] + list(accumulate(g))                                        # P[i] = sum over i' < i
            Q = [0] + list(accumulate(i * x for i, x in enumerate(g)))
            for j, (lo, hi) in enumerate(windows):
                sums[k, b, j] = _words(P[hi] - P[lo]) + _words(Q[hi] - Q[lo])
            T = P[n_bins]
            for l, f in enumerate(levels):
                lo, hi = 0, n_bins                                               # the crossing lies in lo .. hi
                while lo < hi:
                    mid = (lo + hi) // 2
                    if (T - P[mid]) << 32 <= T * f:
                        hi = mid
                    else:
                        lo = mid + 1
                cross[k, b, l] = lo
    return sums, cross
