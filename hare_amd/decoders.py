"""Filter matrices for hare_decode (include/hare_hip.h, "receivers", "Decoding"; Spatial_Partition.decode): numpy on the host, nothing on
the device.  The channel order is this library's -- W X Y Z, then ACN 4..15, SN3D -- not ACN throughout, and the harmonics are the
header's polynomials ("Directional", "Higher orders") evaluated in the header's order, so a decoder built here matches the channels the
receive calls write.  A direction is the unit vector towards where the sound comes from (towards a loudspeaker), in world axes.

  harmonics(dirs, order)                   Y_c(dir_s): [S, C], C = (order + 1)^2
  sampling_decoder(dirs, order)            loudspeaker gains, one tap each: [S, C, 1]
  virtual_speaker_filters(gains, hrirs)    the loudspeaker feeds taken through a head-related impulse response per loudspeaker and ear:
                                           [E, C, T]

No HRIR data is shipped: the caller brings its own set, measured at (or interpolated to) the directions it decodes to."""
from __future__ import annotations

import numpy as np

ORDERS = (0, 1, 2, 3)
DEGREE = np.array([0, 1, 1, 1] + [2] * 5 + [3] * 7)          # l_c of channel c in this library's order


def harmonics(dirs, order: int):
    """float64 [S, C], C = (order + 1)^2: the real spherical harmonics of orders 0..order, SN3D, at the unit vectors dirs [S, 3], in this
    library's channel order: column 0 = W = 1, 1..3 = X, Y, Z = x, y, z, 4.. = ACN 4.. by the polynomials of include/hare_hip.h ("Higher
    orders"), in that order of operations.  dirs must be unit vectors (to 1e-9): they are not normalised here."""
    if order not in ORDERS:
        raise ValueError("order must be 0, 1, 2 or 3")
    a = np.array(dirs, np.float64)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] == 0:
        raise ValueError("dirs must be float64 [S, 3], not empty")
    if not np.isfinite(a).all() or (np.abs(np.sqrt((a * a).sum(axis=1)) - 1.0) > 1e-9).any():
        raise ValueError("dirs must be unit vectors")
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    Y = [np.ones_like(x), x, y, z]
    if order >= 2:
        c3 = np.sqrt(3.0)
        c3h = 0.5 * c3
        xx, yy, zz = x * x, y * y, z * z
        d = xx - yy
        Y += [c3 * (x * y), c3 * (y * z), 1.5 * zz - 0.5, c3 * (x * z), c3h * d]
    if order >= 3:
        c15 = np.sqrt(15.0)
        c15h, c58, c38 = 0.5 * c15, np.sqrt(0.625), np.sqrt(0.375)
        f = 5.0 * zz - 1.0
        Y += [c58 * (y * (3.0 * xx - yy)), c15 * ((x * y) * z), c38 * (y * f), z * (2.5 * zz - 1.5), c38 * (x * f), c15h * (z * d),
              c58 * (x * (xx - 3.0 * yy))]
    return np.stack(Y[:(order + 1) ** 2], axis=1)


def sampling_decoder(dirs, order: int):
    """float64 [S, C, 1]: the sampling decoder of S loudspeakers at dirs [S, 3] as one-tap filters for hare_decode (O = S, T = 1):
    g[s, c] = (2 l_c + 1) Y_c(dir_s) / S, l_c the degree of channel c.  On a layout regular enough for the order (an octahedron at order
    1, a dodecahedron's vertices at order 3) a plane wave from a loudspeaker's direction comes back loudest at that loudspeaker."""
    Y = harmonics(dirs, order)
    S, C = Y.shape
    return (((2.0 * DEGREE[:C] + 1.0)[None, :] * Y) / float(S))[:, :, None]


def virtual_speaker_filters(gains, hrirs):
    """float64 [E, C, T]: h[e, c, :] = sum over s ascending of gains[s, c] * hrirs[s, e, :] -- the loudspeaker feeds of a decoder (gains
    [S, C], or [S, C, 1] as sampling_decoder returns it) played through the head-related impulse responses hrirs [S, E, T] of the S
    loudspeaker directions and E ears, folded into one filter per ear and channel: hare_decode with O = E.  The caller brings hrirs."""
    g, r = np.array(gains, np.float64), np.array(hrirs, np.float64)
    if g.ndim == 3 and g.shape[2] == 1:
        g = g[:, :, 0]
    if g.ndim != 2 or g.size == 0:
        raise ValueError("gains must be float64 [S, C] or [S, C, 1], not empty")
    if r.ndim != 3 or r.size == 0 or r.shape[0] != g.shape[0]:
        raise ValueError("hrirs must be float64 [S, E, T] with the S of gains, not empty")
    h = np.zeros((r.shape[1], g.shape[1], r.shape[2]), np.float64)
    for s in range(g.shape[0]):
        h += g[s][None, :, None] * r[s][:, None, :]
    return h
