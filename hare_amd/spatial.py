"""Spatial room-acoustic parameters from the directional projections of a histogram (include/hare_hip.h, "receivers", "Directional
projection"; Spatial_Partition.hist_project_channels / hist_project_channels_device).  A host convenience in float64, like hare_amd.sti: it
is not part of the contract.  The sums it reads are exact; what it forms from them is not -- the receive loop rounded every signed word
once per deposit, and the divisions here round again.

    table = spatial.window_vectors(n_bins, bin_len, c_sound, [(0, 0.005), (0.005, 0.08), (0, 0.08), (0.08, None)])   # int32 [4, n_bins]
    proj = grid.hist_project_channels(hist, table)                 # uint64 [K, B, 4, C, 2], exact; C = 9 for the second moments
    I, diffuseness = spatial.intensity(proj)                       # float64 [K, B, 4, 3], [K, B, 4]
    lf = spatial.lateral_fraction(proj, [0, 1, 0], early=1, total=2)          # float64 [K, B]; ears along the y axis
"""
from __future__ import annotations

import math

import numpy as np

from .geometry import proj_to_int

SQRT3 = math.sqrt(3.0)


def window_vectors(n_bins: int, bin_len: float, c: float, edges_s):
    """0 / 1 vectors over the bins for time windows: int32 [len(edges_s), n_bins], to be passed as `coef`.  edges_s: pairs (t0, t1) in
    seconds, t1 None for "to the end".  Row j is 1 on the bins whose centre t_i = (i + 0.5) * bin_len / c lies in [t0, t1).  bin_len is a
    PATH LENGTH, as the receive calls take it, in the length unit of c; pass c = 1 with a bin_len in seconds.  Times count from the
    emission: for windows after the direct sound add its arrival time to the edges."""
    n_bins = int(n_bins)
    if n_bins < 1 or not (math.isfinite(bin_len) and bin_len > 0 and math.isfinite(c) and c > 0):
        raise ValueError("n_bins >= 1; bin_len and c finite and > 0")
    t = (np.arange(n_bins, dtype=np.float64) + 0.5) * (float(bin_len) / float(c))
    rows = []
    for t0, t1 in edges_s:
        t1 = math.inf if t1 is None else float(t1)
        if not 0.0 <= float(t0) <= t1:
            raise ValueError("a window is 0 <= t0 <= t1")
        rows.append((t >= float(t0)) & (t < t1))
    if not rows:
        raise ValueError("at least one window")
    return np.ascontiguousarray(np.stack(rows), np.int32)


def _sums(proj, need: int):
    """proj as float64 [K, B, J, C]: from uint64 [K, B, J, C, 2] words or an object array [K, B, J, C] of Python integers, each integer
    rounded once."""
    p = np.asarray(proj)
    if p.dtype != object:
        if p.ndim != 5 or p.shape[4] != 2:
            raise ValueError("proj must be [K, B, J, C] sums or [K, B, J, C, 2] words")
        p = proj_to_int(p)
    if p.ndim != 4:
        raise ValueError("proj must be [K, B, J, C] sums or [K, B, J, C, 2] words")
    if p.shape[3] < need:
        raise ValueError("proj holds %d channels; %d are needed" % (p.shape[3], need))
    return p.astype(np.float64)


def _ratio(a, b):
    """a / b, 0 where b is 0."""
    b = np.asarray(b, np.float64)
    return np.divide(a, b, out=np.zeros(np.broadcast(a, b).shape, np.float64), where=b != 0)


def intensity(proj):
    """The intensity vector per receiver, band and vector (window): I = (X, Y, Z) / W, the energy-weighted mean of the arrival vectors
    (pointing to where the sound came from), float64 [K, B, J, 3], and the diffuseness 1 - |I|, float64 [K, B, J]: 0 for a single plane
    wave, 1 for an isotropic field.  W = 0 gives I = 0 and the diffuseness 1.  Needs channels >= 4."""
    p = _sums(proj, 4)
    I = _ratio(p[..., 1:4], p[..., 0:1])
    return I, 1.0 - np.sqrt((I * I).sum(axis=-1))


def second_moments(proj):
    """The energy-weighted second moments M = sum E a a^T of the arrival vector a = (x, y, z), float64 [K, B, J, 3, 3], in the histogram's
    energy units (divide by channel 0 for the normalised matrix, whose trace is 1).  From channels 0 and 4 .. 8 with the SN3D polynomials
    of "Higher orders" and x^2 + y^2 + z^2 = 1:  zz = (2 Y6 + W) / 3;  xx + yy = W - zz;  xx - yy = 2 Y8 / sqrt(3);  xy = Y4 / sqrt(3);
    yz = Y5 / sqrt(3);  xz = Y7 / sqrt(3).  Needs channels >= 9 (ambisonic order 2), else ValueError."""
    p = _sums(proj, 9)
    W, Y4, Y5, Y6, Y7, Y8 = (p[..., ch] for ch in (0, 4, 5, 6, 7, 8))
    zz = (2.0 * Y6 + W) / 3.0
    s, d = W - zz, 2.0 * Y8 / SQRT3
    xx, yy = 0.5 * (s + d), 0.5 * (s - d)
    xy, yz, xz = Y4 / SQRT3, Y5 / SQRT3, Y7 / SQRT3
    return np.stack([np.stack([xx, xy, xz], -1), np.stack([xy, yy, yz], -1), np.stack([xz, yz, zz], -1)], -2)


def _along(proj, axis):
    """u^T M u per (k, b, j): the energy-weighted (a . u)^2 for the unit vector along `axis`."""
    u = np.asarray(axis, np.float64).reshape(-1)
    if u.shape != (3,) or not np.isfinite(u).all() or not u.any():
        raise ValueError("axis must be a finite non-zero vector [3]")
    u = u / np.sqrt((u * u).sum())
    return np.einsum("i,...ij,j->...", u, second_moments(proj), u)


def lateral_fraction(proj, axis, early: int, total: int):
    """The early lateral energy fraction LF = M_uu(vector `early`) / W(vector `total`), float64 [K, B]: the energy-weighted (a . u)^2 --
    the response of a figure-of-eight microphone along u, the axis through the listener's ears -- over the early window (ISO 3382-1:
    5 .. 80 ms after the direct sound) against the omnidirectional energy of the total window (0 .. 80 ms).  W = 0 gives 0.  Needs
    channels >= 9.  (LFC, with |a . u| in place of its square, is not a polynomial of a and cannot be formed from these channels.)"""
    return _ratio(_along(proj, axis)[:, :, int(early)], _sums(proj, 9)[:, :, int(total), 0])


def lateral_level(proj, axis, window: int, e_ref):
    """The lateral level 10 log10(M_uu(vector `window`) / e_ref) in dB, float64 [K, B] -- with the window 80 ms .. end the late lateral
    level LJ of ISO 3382-1.  e_ref: the reference energy in the histogram's units (the omnidirectional energy of the same source at 10 m
    in a free field), a scalar or anything that broadcasts against [K, B].  No energy gives -inf.  Needs channels >= 9."""
    m = _along(proj, axis)[:, :, int(window)]
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(np.maximum(m, 0.0) / np.asarray(e_ref, np.float64))
