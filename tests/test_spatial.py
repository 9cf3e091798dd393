"""hare_amd.spatial on a histogram with known arrivals, without a GPU: 50 arrivals at known unit directions with energies of 2^30 and
more are deposited into a nine-channel histogram by the header's own rule ("Directional", "Higher orders": word 0 the energy, word ch the
rint of energy x harmonic; the polynomials from tests/ambi_ref.py), projected onto window vectors by the restatement
(tests/project_channels_ref.py), and the intensity vector, the second moments and the lateral fraction are held against direct float sums
of E a, E a a^T and E (a . u)^2.  Tolerance 1e-6 relative: each rint moves a word by at most 1/2 against energies >= 2^30, 2^-31 per
term, which leaves three orders of margin."""
import numpy as np
import pytest

from hare_amd import spatial
from tests.ambi_ref import harmonics
from tests.project_channels_ref import project_channels_ints, project_channels_ref

N_BINS, BIN_LEN, C_SOUND = 40, 1.715, 343.0                                   # 5 ms bins
WINDOWS = [(0.0, 0.005), (0.005, 0.08), (0.0, 0.08), (0.08, None)]
AXES = ([1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [1.0, -2.0, 0.5])                   # two world axes (one not normalised) and an oblique one
RTOL = 1e-6


@pytest.fixture(scope="module")
def scene():
    """(hist [1, n_bins, 1, 9], bins [50], energies [50], directions [50, 3])"""
    rng = np.random.default_rng(2024)
    a = rng.standard_normal((50, 3))
    a /= np.sqrt((a * a).sum(axis=1, keepdims=True))
    a[:, 1] = np.abs(a[:, 1]) * np.where(np.arange(50) % 3 == 0, -1.0, 1.0)   # more from +y than from -y: a clear mean direction
    bins = rng.integers(0, N_BINS, 50)
    bins[:3] = (0, 1, N_BINS - 1)                                             # the direct-sound bin, the first early bin and the last bin are used
    E = np.floor(rng.uniform(2.0 ** 30, 2.0 ** 40, 50))
    hist = np.zeros((1, N_BINS, 1, 9), np.uint64)
    signed = hist[..., 1:].view(np.int64)
    Y = [a[:, 0], a[:, 1], a[:, 2]] + harmonics(a[:, 0], a[:, 1], a[:, 2], order=2)
    for n in range(50):
        hist[0, bins[n], 0, 0] += np.uint64(E[n])
        for ch in range(1, 9):
            signed[0, bins[n], 0, ch - 1] += np.int64(np.rint(E[n] * Y[ch - 1][n]))
    return hist, bins, E, a


def window_of(bins):
    """bool [4, 50]: the arrivals of each window"""
    t = (bins + 0.5) * BIN_LEN / C_SOUND
    return np.stack([(t >= t0) & (t < (np.inf if t1 is None else t1)) for t0, t1 in WINDOWS])


def test_window_vectors_are_zero_one_rows_that_tile_the_bins():
    table = spatial.window_vectors(N_BINS, BIN_LEN, C_SOUND, WINDOWS)
    assert table.dtype == np.int32 and table.shape == (4, N_BINS) and set(table.reshape(-1).tolist()) == {0, 1}
    assert table[0].tolist() == [1] + [0] * (N_BINS - 1) and table[1].tolist() == [0] + [1] * 15 + [0] * (N_BINS - 16)
    assert (table[0] + table[1] == table[2]).all() and (table[2] + table[3] == 1).all()
    for bad in (dict(n_bins=0), dict(bin_len=0.0), dict(c=float("nan")), dict(edges_s=[]), dict(edges_s=[(0.1, 0.05)]), dict(edges_s=[(-1.0, 1.0)])):
        kw = dict(n_bins=N_BINS, bin_len=BIN_LEN, c=C_SOUND, edges_s=WINDOWS)
        kw.update(bad)
        with pytest.raises(ValueError):
            spatial.window_vectors(**kw)


def test_intensity_moments_and_lateral_fraction_equal_the_direct_float_sums(scene):
    hist, bins, E, a = scene
    table = spatial.window_vectors(N_BINS, BIN_LEN, C_SOUND, WINDOWS)
    proj = project_channels_ref(hist, table)                                 # uint64 [1, 1, 4, 9, 2]
    inside = window_of(bins)
    assert inside.sum(axis=1).min() >= 1                                     # no window is empty
    I, diffuse = spatial.intensity(proj)
    M = spatial.second_moments(proj)
    assert I.shape == (1, 1, 4, 3) and diffuse.shape == (1, 1, 4) and M.shape == (1, 1, 4, 3, 3)
    for j in range(4):
        e, v = E[inside[j]], a[inside[j]]
        want_I = (e[:, None] * v).sum(axis=0) / e.sum()
        scale = e.sum()
        assert np.abs(I[0, 0, j] - want_I).max() <= RTOL, (j, I[0, 0, j], want_I)
        assert abs(diffuse[0, 0, j] - (1.0 - np.sqrt((want_I ** 2).sum()))) <= RTOL
        want_M = np.einsum("n,ni,nj->ij", e, v, v)
        assert np.abs(M[0, 0, j] - want_M).max() <= RTOL * scale, (j, M[0, 0, j], want_M)
        assert abs(np.trace(M[0, 0, j]) - scale) <= RTOL * scale            # x^2 + y^2 + z^2 = 1
    assert I[0, 0, 2, 1] > 0.1 and 0.0 < diffuse[0, 0, 2] < 1.0             # the mean direction leans to +y
    total = E[inside[2]].sum()
    for axis in AXES:
        u = np.asarray(axis) / np.linalg.norm(axis)
        want = (E[inside[1]] * (a[inside[1]] @ u) ** 2).sum() / total
        lf = spatial.lateral_fraction(proj, axis, early=1, total=2)
        assert lf.shape == (1, 1) and abs(lf[0, 0] - want) <= RTOL * want, (axis, lf, want)
        late = (E[inside[3]] * (a[inside[3]] @ u) ** 2).sum()
        lj = spatial.lateral_level(proj, axis, 3, total)
        assert abs(lj[0, 0] - 10.0 * np.log10(late / total)) <= 1e-5
    # the object array of Python integers serves as well as the words
    assert np.array_equal(spatial.second_moments(project_channels_ints(hist, table)), M)


def test_too_few_channels_and_malformed_input_are_value_errors(scene):
    hist = scene[0]
    table = spatial.window_vectors(N_BINS, BIN_LEN, C_SOUND, WINDOWS)
    four = project_channels_ref(np.ascontiguousarray(hist[..., :4]), table)
    I, _ = spatial.intensity(four)                                           # four channels carry the intensity ...
    assert np.array_equal(I, spatial.intensity(project_channels_ref(hist, table))[0])
    with pytest.raises(ValueError):
        spatial.second_moments(four)                                         # ... but not the second moments
    with pytest.raises(ValueError):
        spatial.lateral_fraction(four, [0, 1, 0], 1, 2)
    with pytest.raises(ValueError):
        spatial.intensity(project_channels_ref(np.ascontiguousarray(hist[..., 0]), table))
    nine = project_channels_ref(hist, table)
    for axis in ([0, 0, 0], [1, 0], [np.nan, 0, 1]):
        with pytest.raises(ValueError):
            spatial.lateral_fraction(nine, axis, 1, 2)
    with pytest.raises(ValueError):
        spatial.second_moments(nine[0])
    empty = project_channels_ref(np.zeros_like(hist), table)                # no energy: zeros, not NaN
    assert not spatial.intensity(empty)[0].any() and (spatial.intensity(empty)[1] == 1.0).all()
    assert not spatial.lateral_fraction(empty, [0, 1, 0], 1, 2).any()
