"""hare_amd.decoders without a GPU: the filter matrices for hare_decode (include/hare_hip.h, "receivers", "Decoding").  harmonics() is the
header's polynomials ("Higher orders"; restated in tests/ambi_ref.py and once more here, written out) at axis and oblique directions to
1e-15, in this library's channel order -- W X Y Z first, not ACN's W Y Z X; sampling_decoder() on an octahedron at order 1 and on a
dodecahedron's 20 vertices at order 3 sends a plane wave from a loudspeaker's direction back loudest to that loudspeaker; and
virtual_speaker_filters() is the explicit loop over loudspeakers in ascending order, to the bit."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import decoders
from tests import ambi_ref

AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)


def oblique(n=40, seed=3):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def dodecahedron():
    p = (1 + np.sqrt(5.0)) / 2
    v = [[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]
    for a in (-1 / p, 1 / p):
        for b in (-p, p):
            v += [[0, a, b], [a, b, 0], [b, 0, a]]
    v = np.array(v, np.float64)
    assert v.shape == (20, 3)
    return v / np.sqrt(3.0)


def written_out(x, y, z):
    """the sixteen channels as the header writes them, one direction"""
    s3, s15, s58, s38 = np.sqrt(3.0), np.sqrt(15.0), np.sqrt(0.625), np.sqrt(0.375)
    return [1.0, x, y, z,
            s3 * x * y, s3 * y * z, 1.5 * z * z - 0.5, s3 * x * z, 0.5 * s3 * (x * x - y * y),
            s58 * y * (3 * x * x - y * y), s15 * x * y * z, s38 * y * (5 * z * z - 1), z * (2.5 * z * z - 1.5), s38 * x * (5 * z * z - 1),
            0.5 * s15 * z * (x * x - y * y), s58 * x * (x * x - 3 * y * y)]


def test_the_module_is_exported():
    assert H.decoders is decoders and "decoders" in H.__all__


@pytest.mark.parametrize("order", (0, 1, 2, 3))
def test_harmonics_are_the_headers_polynomials(order):
    C = (order + 1) ** 2
    for dirs in (AXES, oblique(), dodecahedron()):
        Y = decoders.harmonics(dirs, order)
        assert Y.shape == (len(dirs), C) and Y.dtype == np.float64
        want = np.array([written_out(*d) for d in dirs])[:, :C]
        assert np.abs(Y - want).max() <= 1e-15
        if order >= 2:          # the restatement the receive tests use: the same operations in the same order, so the same bits
            ref = np.stack(ambi_ref.harmonics(dirs[:, 0], dirs[:, 1], dirs[:, 2], order), axis=1)
            assert Y[:, 4:].tobytes() == ref.tobytes()
    assert decoders.harmonics(dirs, 3)[:, :C].tobytes() == decoders.harmonics(dirs, order).tobytes()          # an order is the head of the next


def test_the_first_four_columns_are_w_x_y_z_not_acn():
    Y = decoders.harmonics(AXES, 3)
    assert (Y[:, 0] == 1).all()
    assert Y[:, 1].tolist() == [1, -1, 0, 0, 0, 0]          # X: ACN would have Y here
    assert Y[:, 2].tolist() == [0, 0, 1, -1, 0, 0]          # Y: ACN would have Z
    assert Y[:, 3].tolist() == [0, 0, 0, 0, 1, -1]          # Z: ACN would have X
    assert Y[:, 6].tolist() == [-0.5, -0.5, -0.5, -0.5, 1, 1] and Y[4, 12] == 1.0          # ACN 6 and 12: the zonal ones
    assert decoders.DEGREE.tolist() == [0, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3]
    # SN3D: the squares of a degree's channels sum to 1 in every direction
    Yo = decoders.harmonics(oblique(), 3) ** 2
    for lo, hi in ((0, 1), (1, 4), (4, 9), (9, 16)):
        assert np.abs(Yo[:, lo:hi].sum(axis=1) - 1).max() < 1e-14


def test_harmonics_refuse_what_is_not_a_list_of_unit_vectors():
    for dirs, order in ((AXES, 4), (AXES, -1), (AXES[0], 1), (AXES[:, :2], 1), (np.zeros((0, 3)), 1), (2 * AXES, 1), (np.full((1, 3), np.nan), 1)):
        with pytest.raises(ValueError):
            decoders.harmonics(dirs, order)


@pytest.mark.parametrize("layout,order", (("octahedron", 1), ("dodecahedron", 3)))
def test_a_plane_wave_from_a_loudspeaker_decodes_loudest_there(layout, order):
    dirs = AXES if layout == "octahedron" else dodecahedron()
    S, C = len(dirs), (order + 1) ** 2
    g = decoders.sampling_decoder(dirs, order)
    assert g.shape == (S, C, 1) and g.dtype == np.float64
    Y = decoders.harmonics(dirs, order)
    assert np.array_equal(g[:, :, 0], (2 * decoders.DEGREE[:C] + 1)[None, :] * Y / S)
    feeds = g[:, :, 0] @ Y.T                                   # feeds[s, w]: loudspeaker s for a plane wave encoded from loudspeaker w
    for w in range(S):
        others = np.delete(feeds[:, w], w)
        assert feeds[w, w] > 0 and (feeds[w, w] > np.abs(others) * 1.5).all(), (w, feeds[:, w])
    assert np.abs(feeds.sum(axis=0) - 1).max() < 1e-12          # and the feeds of a plane wave sum to its pressure: W passes through


def test_virtual_speaker_filters_are_the_explicit_loop():
    rng = np.random.default_rng(8)
    S, C, E, T = 6, 4, 2, 37
    g, r = decoders.sampling_decoder(AXES, 1), rng.standard_normal((S, E, T))
    h = decoders.virtual_speaker_filters(g, r)
    assert h.shape == (E, C, T) and h.dtype == np.float64
    want = np.zeros((E, C, T))
    for e in range(E):
        for c in range(C):
            for t in range(T):
                acc = 0.0
                for s in range(S):
                    acc = acc + g[s, c, 0] * r[s, e, t]
                want[e, c, t] = acc
    assert h.tobytes() == want.tobytes()
    assert decoders.virtual_speaker_filters(g[:, :, 0], r).tobytes() == h.tobytes()          # [S, C] as well as [S, C, 1]
    for bad_g, bad_r in ((g[:5], r), (g, r[:, :, :0]), (g[0], r), (g, r[0]), (np.zeros((S, C, 2)), r)):
        with pytest.raises(ValueError):
            decoders.virtual_speaker_filters(bad_g, bad_r)
