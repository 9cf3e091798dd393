"""hare_amd.sti without a GPU: on a geometric histogram g_i = floor(2^40 r^i) the modulation transfer function formed from the exact
projections (tests/project_ref.py onto sti.mtf_vectors) equals a float64 evaluation of the same discrete sums and the closed form of the
untruncated series; sti() at its three fixed points."""
import math

import numpy as np
import pytest

from hare_amd import sti
from tests.project_ref import project_ref

N_BINS, R = 4096, 0.99          # the truncation term r^n_bins = 1.3e-18, far below 1e-9
BIN_LEN, C_SOUND = 3.43, 343.0  # 10 ms bins


@pytest.fixture(scope="module")
def geometric():
    g = [int(math.floor(2.0 ** 40 * R ** i)) for i in range(N_BINS)]
    hist = np.tile(np.array(g, np.uint64).reshape(1, N_BINS, 1), (1, 1, 7))
    table = sti.mtf_vectors(N_BINS, BIN_LEN, C_SOUND)
    return np.array(g, np.float64), table, sti.mtf(project_ref(hist, table))


def test_the_table_is_ones_cosines_and_sines_at_the_bin_centres():
    t = sti.mtf_vectors(5, BIN_LEN, C_SOUND, freqs=(0.0, 12.5), bits=30)
    assert t.dtype == np.int32 and t.shape == (5, 5) and t.flags.c_contiguous
    assert (t[0] == 1).all() and (t[1] == 1 << 30).all() and (t[3] == 0).all()          # F = 0: cos 1, sin 0
    centres = (np.arange(5) + 0.5) * 0.01
    assert t[2].tolist() == [round(math.cos(2 * math.pi * 12.5 * x) * 2 ** 30) for x in centres]
    assert t[4].tolist() == [round(math.sin(2 * math.pi * 12.5 * x) * 2 ** 30) for x in centres]
    assert sti.mtf_vectors(8, 0.01, 1.0).shape == (29, 8) and len(sti.IEC_FREQS) == 14
    for bad in (dict(bits=31), dict(bits=0), dict(n_bins=0), dict(bin_len=0.0), dict(c_sound=float("nan"))):
        with pytest.raises(ValueError):
            sti.mtf_vectors(**{**dict(n_bins=8, bin_len=0.01, c_sound=1.0), **bad})


def test_mtf_equals_the_float_evaluation_of_the_same_sums(geometric):
    """Bound 1e-8: a coefficient is rounded by at most 2^-31 relative to 2^30, so C and S move by at most 2^-31 T; the float64 sums over
    n_bins <= 4 096 terms add n x 2^-53 = 4.5e-13."""
    g, _, m = geometric
    assert m.shape == (1, 7, 14)
    t = (np.arange(N_BINS) + 0.5) * BIN_LEN / C_SOUND
    for f, F in enumerate(sti.IEC_FREQS):
        want = math.hypot(float(np.sum(g * np.cos(2 * np.pi * F * t))), float(np.sum(g * np.sin(2 * np.pi * F * t)))) / float(np.sum(g))
        print(F, m[0, 0, f], want, abs(m[0, 0, f] - want))
        assert abs(m[0, :, f] - want).max() <= 1e-8, (F, m[0, 0, f], want)


def test_mtf_equals_the_closed_form_of_the_geometric_series(geometric):
    """sum r^i e^{-j w (i + 1/2)} has the modulus |1 / (1 - r e^{-j w})|, so m = (1 - r) / |1 - r e^{-j w}| with w = 2 pi F bin_len / c.
    Bound 1e-9, the cap the truncation term r^n_bins is chosen under (1.3e-18 here).  What else separates the exact projections from the
    series stays under it in the worst case: a coefficient is rounded by at most 1/2, so C and S each move by at most T / 2, that is
    2^-31 of T 2^30, and m by at most sqrt(2) 2^-31 = 6.6e-10; the floor in g moves each word by less than 1, 4 096 in all against
    T = 2^40 / (1 - r) = 1.1e14: 3.7e-11 on the numerator and as much on T.  Together 7.3e-10."""
    _, _, m = geometric
    for f, F in enumerate(sti.IEC_FREQS):
        w = 2 * math.pi * F * BIN_LEN / C_SOUND
        want = (1 - R) / abs(1 - R * complex(math.cos(w), -math.sin(w)))
        print(F, m[0, 0, f], want, abs(m[0, 0, f] - want))
        assert abs(m[0, :, f] - want).max() <= 1e-9, (F, m[0, 0, f], want)
    assert R ** N_BINS < 1e-9


def test_mtf_of_nothing_is_zero_and_accepts_integers():
    p = np.zeros((2, 7, 29, 2), np.uint64)
    assert not sti.mtf(p).any()
    q = np.zeros((1, 1, 3), object)
    q[0, 0] = [5, 3 << 30, -(4 << 30)]
    assert sti.mtf(q)[0, 0, 0] == 1.0                                        # sqrt(9 + 16) / 5
    with pytest.raises(ValueError):
        sti.mtf(np.zeros((1, 7, 28, 2), np.uint64))


def test_sti_at_its_fixed_points():
    ones, zeros = np.ones((3, 7, 14)), np.zeros((7, 14))
    assert np.allclose(sti.sti(ones), 1.0, rtol=0, atol=1e-12) and sti.sti(ones).shape == (3,)
    assert abs(float(sti.sti(zeros))) <= 1e-12
    assert abs(float(sti.sti(ones[0], snr_db=0.0)) - 0.5) <= 1e-12
    assert abs(float(sti.sti(ones[0], snr_db=[0.0] * 7)) - 0.5) <= 1e-12
    assert abs(sum(sti.ALPHA_MALE) - sum(sti.BETA_MALE) - 1.0) <= 1e-12
    with pytest.raises(ValueError):
        sti.sti(np.ones((8, 14)))
