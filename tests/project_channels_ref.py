"""The directional projection of a receive histogram (include/hare_hip.h, "receivers", "Directional projection"), restated in integers:
what hare_hist_project_channels must return, bit for bit.  No floats anywhere.  project_channels_direct is the definition word for word in
Python integers (tiny inputs); project_channels_ref the same through exact int64 matrix products of 16-bit limbs, for the sizes the device
tests use (tests/test_project_channels_cases.py holds the two against each other).  truncating=True is NOT the definition: it weights a
negative word towards zero, the mistake the floor rule excludes, and exists so that the tests can show the cases tell the two apart."""
import numpy as np

from tests.project_ref import M64, _words, to_int  # noqa: F401  (to_int: [..., 2] words -> Python integers, for the callers)


def _hist4(hist):
    """[K, n_bins, B] or [K, n_bins, B, C] -> uint64 [K, n_bins, B, C]."""
    hist = np.asarray(hist, np.uint64)
    return hist[..., None] if hist.ndim == 3 else hist


def project_channels_direct(hist, coef, weight=None, truncating=False):
    """The definition as the header states it.  hist: uint64 [K, n_bins, B] or [K, n_bins, B, C]; coef: int32 [J, n_bins]; weight: uint32
    [n_bins, B] or None.  Returns uint64 [K, B, J, C, 2]: lo, hi."""
    h4 = _hist4(hist)
    K, n_bins, B, C = h4.shape
    h = h4.tolist()
    c = np.asarray(coef, np.int32).tolist()
    w = None if weight is None else np.asarray(weight, np.uint32).tolist()
    proj = np.zeros((K, B, len(c), C, 2), np.uint64)
    for k in range(K):
        for b in range(B):
            for ch in range(C):
                g = []
                for i in range(n_bins):
                    x = h[k][i][b][ch]
                    if ch >= 1 and x >= 1 << 63:
                        x -= 1 << 64                                         # two's complement: (int64)
                    if w is not None:
                        p = x * w[i][b]
                        x = -((-p) >> 32) if truncating and p < 0 else p >> 32    # >> on a Python integer floors towards minus infinity
                    g.append(x)
                for j, cj in enumerate(c):
                    proj[k, b, j, ch] = _words(sum(cj[i] * g[i] for i in range(n_bins)))
    return proj


def _g_limbs(hist, weight, truncating):
    """(sign [K, n_bins, B, C] int64 of +-1, magnitude uint64 of the same shape): g = sign * magnitude.  A signed word is split into sign
    and magnitude |h| <= 2^63; the magnitude is weighted from its 32-bit halves in uint64, exactly.  For a negative word
    floor(-|h| w / 2^32) = -ceil(|h| w / 2^32): the quotient plus one where the product has a remainder -- the remainder's 32 bits are
    ((|h|_lo * w) mod 2^32), since |h|_hi * w * 2^32 contributes none."""
    h = _hist4(hist)
    C = h.shape[3]
    neg = np.zeros(h.shape, bool)
    if C > 1:
        neg[..., 1:] = h[..., 1:] >> np.uint64(63) == 1
    with np.errstate(over="ignore"):
        mag = np.where(neg, (~h) + np.uint64(1), h)                          # |h|: 2^63 for INT64_MIN
    if weight is not None:
        w = np.asarray(weight, np.uint32).astype(np.uint64)[None, :, :, None]
        lo, hi = mag & np.uint64(0xFFFFFFFF), mag >> np.uint64(32)
        low = lo * w                                                         # < 2^64
        q = hi * w + (low >> np.uint64(32))                                  # floor(|h| w / 2^32) <= 2^63: nothing wraps
        rem = (low & np.uint64(0xFFFFFFFF)) != 0
        mag = q + (np.uint64(0) if truncating else (neg & rem).astype(np.uint64))
    return np.where(neg, -1, 1).astype(np.int64), mag


def project_channels_ints(hist, coef, weight=None, truncating=False):
    """The sums themselves, an object array [K, B, J, C] of Python integers.  |g| is split into four 16-bit limbs held as int64 with g's
    sign; one coef.astype(int64) @ limb per limb: every term is below 2^31 * 2^16 = 2^47 in magnitude, so with n_bins <= 2^16 every sum
    stays inside int64 and is exact; the limbs are recombined as Python integers.  (The top limb of |INT64_MIN| = 2^63 is 2^15.)"""
    sign, mag = _g_limbs(hist, weight, truncating)
    K, n_bins, B, C = mag.shape
    if n_bins > 1 << 16:
        raise ValueError("project_channels_ref: n_bins <= 2^16")
    c = np.asarray(coef, np.int32).astype(np.int64)                          # [J, n_bins]
    total = np.zeros((K, B, c.shape[0], C), object)
    for limb in range(4):
        part = ((mag >> np.uint64(16 * limb)) & np.uint64(0xFFFF)).astype(np.int64) * sign      # [K, n_bins, B, C]
        s = np.einsum("ji,kibc->kbjc", c, part)                              # int64, exact
        total = total + s.astype(object) * (1 << (16 * limb))
    return total


def project_channels_ref(hist, coef, weight=None, truncating=False):
    """project_channels_direct, vectorised (project_channels_ints): uint64 [K, B, J, C, 2]."""
    total = project_channels_ints(hist, coef, weight, truncating)
    proj = np.zeros(total.shape + (2,), np.uint64)
    flat = proj.reshape(-1, 2)
    for n, x in enumerate(total.reshape(-1)):
        flat[n] = _words(int(x))
    return proj
