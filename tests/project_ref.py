"""The projection of a receive histogram (include/hare_hip.h, "receivers", "Projection"), restated in integers: what hare_hist_project must
return, bit for bit.  No floats anywhere.  project_direct is the definition word for word in Python integers (tiny inputs); project_ref the
same through exact int64 matrix products of 16-bit limbs, for the sizes the device tests use (tests/test_project_api.py holds the two
against each other)."""
import numpy as np

M64 = (1 << 64) - 1
M128 = (1 << 128) - 1


def _hist(hist):
    hist = np.asarray(hist, np.uint64)
    if hist.ndim == 4:
        hist = hist[..., 0]                      # channel 0, W
    return hist


def _g(hist, weight):
    """g [K, n_bins, B] uint64: h, or floor(h * w / 2^32) as the reduction's restatement forms it, here from 32-bit halves in uint64."""
    h = _hist(hist)
    if weight is None:
        return h
    w = np.asarray(weight, np.uint32).astype(np.uint64)[None]
    lo, hi = h & np.uint64(0xFFFFFFFF), h >> np.uint64(32)
    return hi * w + ((lo * w) >> np.uint64(32))          # (2^32 - 1)^2 + (2^32 - 1) < 2^64: nothing wraps


def _words(x):
    x &= M128                                    # two's complement
    return [x & M64, x >> 64]


def project_direct(hist, coef, weight=None):
    """The definition as the header states it.  hist: uint64 [K, n_bins, B] or [K, n_bins, B, C]; coef: int32 [J, n_bins]; weight: uint32
    [n_bins, B] or None.  Returns uint64 [K, B, J, 2]: lo, hi."""
    h = _hist(hist).tolist()
    K, n_bins, B = _hist(hist).shape
    c = np.asarray(coef, np.int32).tolist()
    w = None if weight is None else np.asarray(weight, np.uint32).tolist()
    proj = np.zeros((K, B, len(c), 2), np.uint64)
    for k in range(K):
        for b in range(B):
            g = [h[k][i][b] if w is None else (h[k][i][b] * w[i][b]) >> 32 for i in range(n_bins)]
            for j, cj in enumerate(c):
                proj[k, b, j] = _words(sum(cj[i] * g[i] for i in range(n_bins)))
    return proj


def project_ints(hist, coef, weight=None):
    """The sums themselves, an object array [K, B, J] of Python integers.  g is split into four 16-bit limbs held as int64; one
    coef.astype(int64) @ limb per limb: every term is below 2^31 * 2^16 = 2^47, so with n_bins <= 2^16 every sum stays inside int64 and is
    exact; the limbs are recombined as Python integers."""
    g = _g(hist, weight)
    K, n_bins, B = g.shape
    if n_bins > 1 << 16:
        raise ValueError("project_ref: n_bins <= 2^16")
    c = np.asarray(coef, np.int32).astype(np.int64)                          # [J, n_bins]
    total = np.zeros((K, B, c.shape[0]), object)
    for limb in range(4):
        part = ((g >> np.uint64(16 * limb)) & np.uint64(0xFFFF)).astype(np.int64)          # [K, n_bins, B]
        s = np.einsum("ji,kib->kbj", c, part)                                # int64, exact
        total = total + s.astype(object) * (1 << (16 * limb))
    return total


def project_ref(hist, coef, weight=None):
    """project_direct, vectorised (project_ints): uint64 [K, B, J, 2]."""
    total = project_ints(hist, coef, weight)
    proj = np.zeros(total.shape + (2,), np.uint64)
    flat = proj.reshape(-1, 2)
    for n, x in enumerate(total.reshape(-1)):
        flat[n] = _words(int(x))
    return proj


def to_int(proj):
    """[..., 2] (lo, hi) words -> object array of Python integers."""
    p = np.asarray(proj, np.uint64)
    v = p[..., 0].astype(object) + p[..., 1].astype(object) * (1 << 64)
    return v - (p[..., 1] >> np.uint64(63)).astype(object) * (1 << 128)
