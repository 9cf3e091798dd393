"""The rendering of a receive histogram (include/hare_hip.h, "receivers", "Rendering"), restated in numpy: what hare_hist_render must
return, bit for bit.  Elementwise over (k, b, n) -- numpy's multiply, add, divide and sqrt are IEEE operations, one rounding each, never
fused -- with Python loops over t, j and b, so every sum runs in the header's order."""
import numpy as np

from tests.scatter_ref import G, mix

MASK = (1 << 64) - 1


def signs(seed, K, count):
    """s(k, i), i = 0 .. count - 1: float64 [K, count] of +-1.0."""
    with np.errstate(over="ignore"):
        base = mix(mix(np.uint64(int(seed) & MASK) + G) ^ np.arange(K, dtype=np.uint64))
        z = mix(base[:, None] + np.arange(count, dtype=np.uint64)[None, :] * G)
    return np.where((z >> np.uint64(63)) != 0, -1.0, 1.0)


def weighted(h, weight):
    """g of "Reduction": h, or floor(h * weight / 2^32) from 32-bit pieces (no overflow: the result is below 2^64)."""
    if weight is None:
        return h
    w = np.asarray(weight, np.uint32).astype(np.uint64)[None]
    return (h >> np.uint64(32)) * w + (((h & np.uint64(0xFFFFFFFF)) * w) >> np.uint64(32))


def render_ref(hist, taps, M, frac_bits, seed=0, weight=None):
    """hist: uint64 [K, n_bins, B] or [K, n_bins, B, C]; taps: float64 [B, T]; weight: uint32 [n_bins, B] or None.
    Returns float64 [K, C, n_bins * M]."""
    hist = np.asarray(hist, np.uint64)
    if hist.ndim == 3:
        hist = hist[..., None]
    taps = np.asarray(taps, np.float64)
    K, nb, B, C = hist.shape
    T, N = taps.shape[1], nb * M
    with np.errstate(all="ignore"):
        s = signs(seed, K, N + T - 1)
        y = taps[None, :, 0, None] * s[:, None, T - 1:T - 1 + N]                        # [K, B, N]
        for t in range(1, T):
            y = y + taps[None, :, t, None] * s[:, None, T - 1 - t:T - 1 - t + N]
        yb = y.reshape(K, B, nb, M)
        p = yb[..., 0] * yb[..., 0]
        for j in range(1, M):
            p = p + yb[..., j] * yb[..., j]
        p = p.transpose(0, 2, 1)                                                         # [K, n_bins, B]
        hW = hist[..., 0]
        e = np.ldexp(weighted(hW, weight).astype(np.float64), -int(frac_bits))
        a = np.where((p > 0.0) & (e > 0.0), np.sqrt(e / np.where(p > 0.0, p, 1.0)), 0.0)
        out = np.zeros((K, C, N))
        for ch in range(C):
            if ch == 0:
                r = np.ones((K, nb, B))
            else:
                r = np.where(hW != 0, hist[..., ch].view(np.int64).astype(np.float64) / np.where(hW != 0, hW, 1).astype(np.float64), 0.0)
            gain = np.repeat(a * r, M, axis=1)                                           # [K, N, B]: constant across a bin
            z = gain[:, :, 0] * y[:, 0]
            for b in range(1, B):
                z = z + gain[:, :, b] * y[:, b]
            out[:, ch] = z
    return out
