"""numpy restatement of the higher-order receivers (include/hare_hip.h, "receivers", "Higher orders"): HARE_RECEIVE_ORDER2 and
HARE_RECEIVE_ORDER3 widen a directional histogram word from four channels to C = 9 or 16.  Channels 0..3 are W, X, Y, Z exactly as
"Directional" defines them; channels 4..15 are the real spherical harmonics ACN 4..15 in SN3D normalisation, polynomials of the same
arrival vector a = (x, y, z), FP64, one operation at a time in the order written in harmonics() below.

Everything that does not change is tests/receive_ref.py's (and, for the source paths, direct_ref / image_ref / image2_ref, which share its
deposit): the loop, the receiver step, the rain, the rules, the maps.  What changes is the deposit, and that is here: deposit() adds the
first four channels through receive_ref.deposit and the channels 4 .. C - 1 itself.  The reference modules create their own four-channel
histograms, so the higher channels are collected beside them: inside `with higher_order(order) as extra:` every deposit the reference
modules make goes through deposit() below, and extra.words holds [K, n_bins, B, C - 4], to be joined behind the four (join())."""
import contextlib

import numpy as np

from tests import direct_ref, image2_ref, image_ref, receive_ref
from tests.receive_ref import magnitude, signed_words

FIRST_ORDER_DEPOSIT = receive_ref.deposit           # the four channels' deposit, whatever higher_order() has put in its place

CHANNELS = {1: 4, 2: 9, 3: 16}

# the six constants: correctly rounded square roots and their exact halves
C3 = np.sqrt(np.float64(3.0))
C3H = np.float64(0.5) * C3
C15 = np.sqrt(np.float64(15.0))
C15H = np.float64(0.5) * C15
C58 = np.sqrt(np.float64(0.625))
C38 = np.sqrt(np.float64(0.375))
CONSTANTS = dict(c3=C3, c3h=C3H, c15=C15, c15h=C15H, c58=C58, c38=C38)


def harmonics(x, y, z, order=3):
    """Y4 .. Y8 (order 2) or Y4 .. Y15 (order 3) of the arrival vector, a list of arrays shaped like x."""
    x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
    with np.errstate(all="ignore"):
        xx = x * x
        yy = y * y
        zz = z * z
        d = xx - yy
        out = [C3 * (x * y), C3 * (y * z), 1.5 * zz - 0.5, C3 * (x * z), C3H * d]
        if order >= 3:
            f = 5.0 * zz - 1.0
            out += [C58 * (y * (3.0 * xx - yy)), C15 * ((x * y) * z), C38 * (y * f), z * (2.5 * zz - 1.5), C38 * (x * f), C15H * (z * d),
                    C58 * (x * (xx - 3.0 * yy))]
    return out


class Extra:
    """The channels 4 .. C - 1 of every deposit made inside higher_order(): words [K, n_bins, B, C - 4] uint64 (None before the first)."""

    def __init__(self, order):
        self.order = order
        self.words = None


def deposit(extra, hist, k, bins, v, frac_bits, arrival, counts=None, tallies=None):
    """receive_ref.deposit on the four channels of hist [K, n_bins, B, 4], then hist's channels 4 .. C - 1 into extra.words:
    words[k, bin, b, ch - 4] += (uint64) s_ch with s_ch the "Directional" rule on m_b * Y_ch."""
    if hist.ndim != 4:
        raise ValueError("the higher orders stand on a directional histogram")
    kept = []

    def arrival_once():
        kept.append(arrival())
        return kept[0]
    FIRST_ORDER_DEPOSIT(hist, k, bins, v, frac_bits, arrival_once, counts, tallies)
    if extra.words is None:
        extra.words = np.zeros(hist.shape[:3] + (CHANNELS[extra.order] - 4,), np.uint64)
    m = magnitude(v, frac_bits)
    Y = harmonics(*kept[0], order=extra.order)
    with np.errstate(over="ignore"):
        for b in range(hist.shape[2]):
            for j, y in enumerate(Y):
                np.add.at(extra.words[k, :, b, j], bins, signed_words(m[b], y))


@contextlib.contextmanager
def higher_order(order):
    """Inside, the deposits of receive_ref, direct_ref, image_ref and image2_ref are deposit() above; yields the Extra they fill."""
    extra = Extra(order)
    mods = (receive_ref, direct_ref, image_ref, image2_ref)
    saved = [m.deposit for m in mods]

    def patched(hist, k, bins, v, frac_bits, arrival, counts=None, tallies=None):
        deposit(extra, hist, k, bins, v, frac_bits, arrival, counts, tallies)
    for m in mods:
        m.deposit = patched
    try:
        yield extra
    finally:
        for m, f in zip(mods, saved):
            m.deposit = f


def join(hist4, extra):
    """[K, n_bins, B, 4] and the Extra of the same deposits -> [K, n_bins, B, C]."""
    C = CHANNELS[extra.order]
    words = extra.words if extra.words is not None else np.zeros(hist4.shape[:3] + (C - 4,), np.uint64)
    return np.ascontiguousarray(np.concatenate([hist4, words], axis=3))


def run(order, fn, *args, **kw):
    """fn(*args, **kw) -- a reference function that returns a dict with "hist" or a tuple whose first item is the histogram -- at
    `order`: the same result with the histogram widened to C channels.  order 1 is fn itself."""
    if order == 1:
        return fn(*args, **kw)
    with higher_order(order) as extra:
        out = fn(*args, **kw)
    if isinstance(out, dict):
        out = dict(out)
        out["hist"] = join(out["hist"], extra)
        return out
    return (join(out[0], extra),) + tuple(out[1:])


def signed(hist):
    """The channels 1 .. C - 1 of a histogram [..., C] as int64 (a view)."""
    return hist[..., 1:].view(np.int64)
