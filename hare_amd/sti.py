"""The speech transmission index (IEC 60268-16) from the projections of a histogram (include/hare_hip.h, "receivers", "Projection";
Spatial_Partition.hist_project / hist_project_device).  A host convenience that produces and reads data, like band_taps: it is not part of
the contract, and whatever int32 vectors a caller projects onto are the definition's c_j.

    table = sti.mtf_vectors(n_bins, bin_len, c_sound)          # int32 [29, n_bins]: ones, 14 cosines, 14 sines
    proj = grid.hist_project(hist, table)                      # uint64 [K, 7, 29, 2], exact
    value = sti.sti(sti.mtf(proj))                             # float64 [K]
"""
from __future__ import annotations

import math

import numpy as np

from .geometry import proj_to_int

# the 14 modulation frequencies of IEC 60268-16, Hz: third octaves from 0.63 to 12.5
IEC_FREQS = (0.63, 0.8, 1.0, 1.25, 1.6, 2.0, 2.5, 3.15, 4.0, 5.0, 6.3, 8.0, 10.0, 12.5)
# IEC 60268-16:2011, Annex A, table A.3, "MTI octave band weighting factors", male speech: alpha for the octave bands 125 Hz .. 8 kHz and
# the redundancy factors beta for the pairs of adjacent bands 125/250 .. 4k/8k.  sum(alpha) - sum(beta) = 1
ALPHA_MALE = (0.085, 0.127, 0.230, 0.233, 0.309, 0.224, 0.173)
BETA_MALE = (0.085, 0.078, 0.065, 0.011, 0.047, 0.095)


def mtf_vectors(n_bins: int, bin_len: float, c_sound: float, freqs=IEC_FREQS, bits: int = 30):
    """The coefficient table of the modulation transfer function: int32 [2 F + 1, n_bins] -- a row of ones (the total T), then per
    frequency round(2^bits cos(2 pi f t_i)), then per frequency round(2^bits sin(2 pi f t_i)), at the bin centres
    t_i = (i + 0.5) * bin_len / c_sound.  bin_len is a PATH LENGTH, as the receive calls take it (a bin holds the arrivals whose path
    length lies in [i, i + 1) * bin_len), in the length unit of c_sound; pass c_sound = 1 with a bin_len in seconds.  freqs in Hz;
    1 <= bits <= 30, so that 2^bits fits an int32."""
    n_bins, bits = int(n_bins), int(bits)
    f = np.asarray(freqs, np.float64).reshape(-1)
    if n_bins < 1 or not 1 <= bits <= 30:
        raise ValueError("n_bins >= 1 and 1 <= bits <= 30")
    if not (math.isfinite(bin_len) and bin_len > 0 and math.isfinite(c_sound) and c_sound > 0 and np.isfinite(f).all() and (f >= 0).all()):
        raise ValueError("bin_len and c_sound are finite and > 0, freqs finite and >= 0")
    t = (np.arange(n_bins, dtype=np.float64) + 0.5) * (float(bin_len) / float(c_sound))
    phase = 2.0 * np.pi * f[:, None] * t[None, :]
    scale = float(1 << bits)
    table = np.concatenate([np.ones((1, n_bins)), np.rint(np.cos(phase) * scale), np.rint(np.sin(phase) * scale)])
    return np.ascontiguousarray(table, np.int32)


def mtf(proj, bits: int = 30):
    """The modulation transfer function m = sqrt(C^2 + S^2) / (T * 2^bits) from the projections onto mtf_vectors' table: proj is what
    hist_project returns, uint64 [K, B, 2 F + 1, 2] or the object array [K, B, 2 F + 1] of Python integers.  Returns float64 [K, B, F].
    The quotient (C^2 + S^2) / (T * 2^bits)^2 is formed in Python integers and rounded once; T = 0 gives 0."""
    p = np.asarray(proj)
    if p.dtype != object:
        p = proj_to_int(p)
    if p.ndim != 3 or p.shape[2] < 3 or p.shape[2] % 2 == 0:
        raise ValueError("proj must be [K, B, 2 F + 1] sums (or [K, B, 2 F + 1, 2] words)")
    K, B, n = p.shape
    F = (n - 1) // 2
    out = np.zeros((K, B, F), np.float64)
    for k in range(K):
        for b in range(B):
            T = int(p[k, b, 0]) << int(bits)
            if T <= 0:
                continue
            for f in range(F):
                C, S = int(p[k, b, 1 + f]), int(p[k, b, 1 + F + f])
                out[k, b, f] = math.sqrt((C * C + S * S) / (T * T))
    return out


def sti(m, alpha=ALPHA_MALE, beta=BETA_MALE, snr_db=None):
    """The speech transmission index from modulation transfer values m, float [..., 7, F] (seven octave bands 125 Hz .. 8 kHz, F
    modulation frequencies): m is multiplied by the noise factor 1 / (1 + 10^(-SNR / 10)) where snr_db is given (a number, or seven, per
    band); the effective signal-to-noise ratio 10 log10(m / (1 - m)) is clipped to +-15 dB; the transmission index is (SNR + 15) / 30;
    its mean over F is the band's MTI; and STI = sum alpha_b MTI_b - sum beta_b sqrt(MTI_b MTI_b+1).  alpha and beta default to the male
    weights of IEC 60268-16.  Level-dependent auditory masking and the absolute reception threshold of the standard are LEFT OUT: this is
    the index of the room's (and the given noise's) modulation reduction alone.  Returns float64 [...]."""
    m = np.asarray(m, np.float64)
    a, bt = np.asarray(alpha, np.float64).reshape(-1), np.asarray(beta, np.float64).reshape(-1)
    if m.ndim < 2 or m.shape[-2] != 7 or a.size != 7 or bt.size != 6:
        raise ValueError("sti needs seven octave bands: m [..., 7, F], seven alpha, six beta")
    if snr_db is not None:
        snr = np.broadcast_to(np.asarray(snr_db, np.float64), (7,))
        m = m * (1.0 / (1.0 + 10.0 ** (-snr / 10.0)))[:, None]
    m = np.clip(m, 0.0, 1.0)
    with np.errstate(divide="ignore"):
        snr_eff = np.clip(10.0 * np.log10(m / (1.0 - m)), -15.0, 15.0)          # m = 0 gives -inf, m = 1 gives +inf: both clipped
    mti = ((snr_eff + 15.0) / 30.0).mean(axis=-1)
    return (mti * a).sum(axis=-1) - (np.sqrt(mti[..., :-1] * mti[..., 1:]) * bt).sum(axis=-1)
