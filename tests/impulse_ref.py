"""The impulses of a per-sample receive histogram (include/hare_hip.h, "receivers", "Impulses"), restated in numpy: what hare_hist_impulses
must return, bit for bit.  Python loops over k, over b and over the entries of a band in ascending bin; an entry's term is added to the
outputs it reaches elementwise -- numpy's multiply, add, divide and sqrt are IEEE operations, one rounding each, never fused -- so every
output's sum runs in the header's order: bands ascending and, within a band, bins ascending, terms without an entry or with a tap out of
range never formed.  `bands` and `bins` turn the order round: what a kernel that walked the other way would compute."""
import numpy as np

from tests.render_ref import weighted


def entries(hist, weight=None):
    """g uint64 [K, n_bins, B]: the weighted W word; an entry exists where it is not 0"""
    hist = np.ascontiguousarray(hist, np.uint64)
    if hist.ndim == 3:
        hist = hist[..., None]
    return weighted(hist[..., 0], weight)


def gains(hist, frac_bits, weight=None):
    """gain_ch float64 [K, n_bins, B, C] (meaningless where there is no entry) and the entries' mask [K, n_bins, B]"""
    hist = np.ascontiguousarray(hist, np.uint64)
    if hist.ndim == 3:
        hist = hist[..., None]
    g = entries(hist, weight)
    hW = hist[..., 0]
    with np.errstate(all="ignore"):
        a = np.sqrt(np.ldexp(g.astype(np.float64), -int(frac_bits)))
        r = hist.view(np.int64).astype(np.float64) / np.where(hW != 0, hW, 1).astype(np.float64)[..., None]
        r[..., 0] = 1.0
        return a[..., None] * r, g != 0


def impulse_ref(hist, taps, frac_bits, n0=0, n_out=None, weight=None, out=None, add=0, bands="ascending", bins="ascending"):
    """hist: uint64 [K, n_bins, B] or [K, n_bins, B, C]; taps: float64 [B, T]; weight: uint32 [n_bins, B] or None.  out None: returns
    float64 [K, C, n_out].  out float64 [K, C, stride >= n_out]: a copy of it is returned with the first n_out words of every row replaced
    (add 0) or added onto (add 1), the rest as it was."""
    hist = np.ascontiguousarray(hist, np.uint64)
    if hist.ndim == 3:
        hist = hist[..., None]
    taps = np.asarray(taps, np.float64)
    K, nb, B, C = hist.shape
    T = taps.shape[1]
    n0 = int(n0)
    n_out = nb + T - 1 - n0 if n_out is None else int(n_out)
    assert taps.shape[0] == B and 0 <= n0 and 1 <= n_out and n0 + n_out <= nb + T - 1
    gain, there = gains(hist, frac_bits, weight)
    z = np.zeros((K, C, n_out))                                           # +0.0
    with np.errstate(all="ignore"):
        for k in range(K):
            for b in (range(B) if bands == "ascending" else range(B - 1, -1, -1)):
                at = np.nonzero(there[k, :, b])[0]
                for i in (at if bins == "ascending" else at[::-1]):
                    lo, hi = max(int(i), n0), min(int(i) + T - 1, n0 + n_out - 1)          # the outputs the entry reaches, within the window
                    if lo > hi:
                        continue
                    term = gain[k, i, b, :, None] * taps[b, None, lo - i:hi - i + 1]
                    z[k, :, lo - n0:hi - n0 + 1] = z[k, :, lo - n0:hi - n0 + 1] + term
        if out is None:
            return z
        res = np.array(out, np.float64)
        assert res.shape[:2] == (K, C) and res.shape[2] >= n_out
        res[..., :n_out] = res[..., :n_out] + z if add else z
    return res
