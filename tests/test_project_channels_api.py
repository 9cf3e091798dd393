"""The directional projection of a histogram (include/hare_hip.h, "receivers", "Directional projection") without a GPU, in the manner of
tests/test_project_api.py: the two exports are bound and declared; every refusal of the header is HARE_E_INVALID, in the header's order,
with a message that names the call; the output is `channels` times the projection's, which the overlap check shows; behind the checks a
GPU-less host answers HARE_E_NODEVICE; and the Python mirror checks its shapes."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi

NEW = ("hare_hist_project_channels_device", "hare_hist_project_channels")


@pytest.fixture(scope="module")
def grid():
    m = H.scenes.shoebox()
    return H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)


def test_new_symbols_are_exported_bound_and_declared():
    hdr = open(capi.os.path.join(capi.os.path.dirname(capi._HERE), "include", "hare_hip.h")).read()
    raw = capi.C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in capi.SYMBOLS, name
        assert getattr(capi.lib, name).argtypes == capi.SYMBOLS[name][1]
        assert f"HARE_API int {name}(" in hdr, name
    assert "Directional projection (hare_hist_project_channels_device, hare_hist_project_channels)" in hdr
    assert hdr.index(" * Projection (") < hdr.index(" * Directional projection (") < hdr.index(" * Rendering (")
    assert "LFC" in hdr and "is not offered" in hdr


ARENA = np.zeros(1 << 16, np.uint64)          # any non-null addresses: nothing is dereferenced before the checks pass
A0 = ARENA.ctypes.data


def call(grid, dev, K=2, n_bins=8, B=1, channels=4, hist=A0, weight=None, J=3, coef=A0 + 65536, proj=A0 + 131072):
    """Either call on raw addresses: (rc, message)."""
    if dev:
        rc = capi.lib.hare_hist_project_channels_device(grid._h, K, n_bins, B, channels, hist, weight, J, coef, proj, None)
    else:
        rc = capi.lib.hare_hist_project_channels(grid._h, K, n_bins, B, channels, hist, weight, J, coef, proj)
    return rc, capi.last_error()


SHAPE = [dict(K=0), dict(K=65537), dict(n_bins=0), dict(n_bins=-1), dict(B=0), dict(B=9), dict(channels=0), dict(channels=2), dict(channels=3),
         dict(channels=5), dict(K=65536, n_bins=1025, B=2, channels=1), dict(K=4096, n_bins=4097, B=2, channels=4)]
VECTORS = [dict(J=0), dict(J=-1), dict(J=33)]
NULLS = [dict(hist=None), dict(coef=None), dict(proj=None)]
# with four channels proj is 2 x 1 x 3 x 4 x 2 x 8 = 384 bytes (the projection's 96 times four), hist 512, coef 96, weight 32
OVERLAPS = [dict(proj=A0), dict(proj=A0 + 504), dict(hist=A0 + 131072 + 376), dict(proj=A0 + 65536 + 92), dict(weight=A0 + 131072 + 383),
            dict(weight=A0 + 131072 - 31)]
REFUSED = SHAPE + VECTORS + NULLS + OVERLAPS


def case_id(kw):
    """A case's name; an address as its offset in the arena, so that the name is the same in every process"""
    return ",".join(f"{k}=A0+{v - A0}" if isinstance(v, int) and v >= A0 else f"{k}={v}" for k, v in kw.items())[:50]


@pytest.mark.parametrize("dev", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("kw", REFUSED, ids=case_id)
def test_every_refusal_is_invalid_and_names_the_call(grid, kw, dev):
    rc, msg = call(grid, dev, **kw)
    assert rc == capi.HARE_E_INVALID, (kw, rc, msg)
    assert msg.startswith("hare_hist_project_channels_device:" if dev else "hare_hist_project_channels:"), msg


def test_a_null_scene_is_refused():
    assert capi.lib.hare_hist_project_channels(None, 2, 8, 1, 4, A0, None, 3, A0 + 65536, A0 + 131072) == capi.HARE_E_INVALID
    assert capi.lib.hare_hist_project_channels_device(None, 2, 8, 1, 4, A0, None, 3, A0 + 65536, A0 + 131072, None) == capi.HARE_E_INVALID


@pytest.mark.parametrize("dev", (False, True), ids=("host", "device"))
def test_the_refusals_come_in_the_headers_order_and_the_output_has_every_channel(grid, dev):
    """Shape, then J, then null buffers, then overlap: of two faults the earlier group's message is the one returned."""
    told = {"shape": ("K out of range", "n_bins must be", "bands out of range", "channels must be", "exceeds 2^27"), "J": ("J out of range",),
            "null": ("null histogram",), "overlap": ("must not overlap",)}
    groups = (("shape", SHAPE), ("J", VECTORS), ("null", NULLS), ("overlap", OVERLAPS))
    for a, (first, kws_a) in enumerate(groups):
        for kw_a in kws_a:
            _, msg = call(grid, dev, **kw_a)
            assert any(t in msg for t in told[first]), (kw_a, msg)
            for later, kws_b in groups[a + 1:]:
                for kw_b in kws_b:
                    if set(kw_a) & set(kw_b):
                        continue
                    rc, msg = call(grid, dev, **kw_a, **kw_b)
                    assert rc == capi.HARE_E_INVALID and any(t in msg for t in told[first]), (kw_a, kw_b, msg)
    # the output's size is K x B x J x channels x 16 bytes: a histogram 96 bytes behind proj's start is clear of the projection's output
    # and inside this call's -- refused at four channels, and past every check at one
    rc, msg = call(grid, dev, hist=A0 + 131072 + 96)
    assert rc == capi.HARE_E_INVALID and "must not overlap" in msg
    if H.device_count() == 0:
        assert call(grid, dev, channels=1, hist=A0 + 131072 + 96)[0] == capi.HARE_E_NODEVICE
        # adjacent buffers do not overlap, and a weight beside the output is fine: these get past every check
        for kw in (dict(proj=A0 + 512), dict(proj=A0 + 65536 + 96), dict(weight=A0 + 131072 + 384), dict(weight=A0 + 131072 - 32),
                   dict(channels=9), dict(channels=16, B=8)):
            rc, msg = call(grid, dev, **kw)
            assert rc == capi.HARE_E_NODEVICE, (kw, rc, msg)


@pytest.mark.skipif(H.device_count() > 0, reason="a GPU is present")
def test_without_a_device_the_calls_answer_nodevice(grid):
    h = np.ones((2, 8, 1, 4), np.uint64)
    c = np.ones((3, 8), np.int32)
    with pytest.raises(H.HareError) as ei:
        grid.hist_project_channels(h, c)
    assert ei.value.code == capi.HARE_E_NODEVICE
    with pytest.raises(H.HareError) as ei:
        grid.hist_project_channels_device(2, 8, 1, 4, A0, 3, A0 + 65536, A0 + 131072)
    assert ei.value.code == capi.HARE_E_NODEVICE
    for J in (1, 32):                                                        # the ends of the range are inside it
        assert call(grid, True, J=J)[0] == capi.HARE_E_NODEVICE


def test_the_python_wrapper_checks_shapes_and_never_wraps_a_coefficient(grid):
    h = np.ones((2, 8, 1, 9), np.uint64)
    for bad in (np.ones((3, 7), np.int32), np.ones(8, np.int32), np.ones((0, 8), np.int32), np.full((1, 8), 1 << 31, np.int64),
                np.full((1, 8), -(1 << 31) - 1, np.int64), np.ones((1, 8), np.float64)):
        with pytest.raises(ValueError):
            grid.hist_project_channels(h, bad)
    for bad in (np.ones((2, 8), np.uint64), np.ones((2, 8, 1, 5), np.uint64)):
        with pytest.raises(ValueError):
            grid.hist_project_channels(bad, np.ones((1, 8), np.int32))
    with pytest.raises(ValueError):
        grid.hist_project_channels(h, np.ones((1, 8), np.int32), weight=np.ones((8, 2), np.uint32))
