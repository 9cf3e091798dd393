"""The rendering of a histogram (include/hare_hip.h, "receivers", "Rendering") without a GPU: the two exports are bound and declared; every
refusal of the header is HARE_E_INVALID with a message that names the call, from the host call and from the device call; behind the checks
a GPU-less host answers HARE_E_NODEVICE."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi

NEW = ("hare_hist_render_device", "hare_hist_render")


@pytest.fixture(scope="module")
def grid():
    m = H.scenes.shoebox()
    return H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)


def test_new_symbols_are_exported_bound_and_declared():
    hdr = open(capi.os.path.join(capi.os.path.dirname(capi._HERE), "include", "hare_hip.h")).read()
    for name in NEW:
        assert name in capi.SYMBOLS, name
        assert getattr(capi.lib, name).argtypes == capi.SYMBOLS[name][1]
        assert f"HARE_API int {name}(" in hdr, name
    assert "Rendering (hare_hist_render_device, hare_hist_render)" in hdr


BUF = np.zeros(1 << 16, np.uint64)                   # 512 KiB the calls may point into: nothing is dereferenced before the checks pass
A = BUF.ctypes.data


def call(g, device, K=2, n_bins=8, B=2, channels=4, hist=A, weight=None, frac_bits=20, M=4, T=3, taps=A + (1 << 17), out=A + (1 << 18)):
    """Either call with every argument replaceable: (rc, message).  The good arguments: hist 1 KiB at A, taps 48 bytes at A + 128 KiB,
    out 2 KiB at A + 256 KiB."""
    if device:
        rc = capi.lib.hare_hist_render_device(g._h, K, n_bins, B, channels, hist, weight, frac_bits, M, T, taps, 7, out, None)
    else:
        rc = capi.lib.hare_hist_render(g._h, K, n_bins, B, channels, hist, weight, frac_bits, M, T, taps, 7, out)
    return rc, capi.last_error()


REFUSED = [dict(K=0), dict(K=65537), dict(n_bins=0), dict(n_bins=-1), dict(B=0), dict(B=9), dict(channels=0), dict(channels=2), dict(channels=5),
           dict(channels=17), dict(K=65536, n_bins=1025, B=2, channels=1), dict(K=4096, n_bins=4096, B=2, channels=4),
           dict(M=0), dict(M=1025), dict(M=-1), dict(T=0), dict(T=1025), dict(frac_bits=-1), dict(frac_bits=63),
           dict(K=65536, n_bins=128, B=1, channels=16, M=3),                  # the histogram fits (2^27 words), the output does not
           dict(K=1024, n_bins=1024, B=1, channels=1, M=257),
           dict(hist=None), dict(taps=None), dict(out=None),
           dict(out=A), dict(out=A + 1016), dict(out=A + (1 << 17) - 2040), dict(out=A + (1 << 17) + 40),
           dict(weight=A + (1 << 18) + 2040)]


def case_id(kw):
    """A pointer into BUF is named by its offset from A: the address differs from process to process, a test's name must not"""
    return ",".join(f"{k}=A+{v - A}" if k in ("hist", "taps", "out", "weight") and v is not None else f"{k}={v}" for k, v in kw.items())[:60]


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("kw", REFUSED, ids=case_id)
def test_every_refusal_is_invalid_and_names_the_call(grid, kw, device):
    rc, msg = call(grid, device, **kw)
    assert rc == capi.HARE_E_INVALID, (kw, rc, msg)
    assert msg.startswith("hare_hist_render_device:" if device else "hare_hist_render:"), msg


def test_a_null_scene_is_refused():
    assert capi.lib.hare_hist_render(None, 2, 8, 2, 4, A, None, 20, 4, 3, A + (1 << 17), 7, A + (1 << 18)) == capi.HARE_E_INVALID
    assert capi.lib.hare_hist_render_device(None, 2, 8, 2, 4, A, None, 20, 4, 3, A + (1 << 17), 7, A + (1 << 18), None) == capi.HARE_E_INVALID


def test_the_checks_come_in_the_headers_order(grid):
    for device in (False, True):
        assert "K out of range" in call(grid, device, K=0, M=0, frac_bits=99, hist=None)[1]
        assert "M out of range" in call(grid, device, M=0, frac_bits=99, hist=None)[1]
        assert "T out of range" in call(grid, device, T=0, frac_bits=99, hist=None)[1]
        assert "frac_bits" in call(grid, device, frac_bits=99, hist=None, K=65536, n_bins=128, B=1, channels=16, M=3)[1]
        assert "2^28" in call(grid, device, hist=None, K=65536, n_bins=128, B=1, channels=16, M=3)[1]
        assert "null" in call(grid, device, hist=None, out=A)[1]
        assert "overlap" in call(grid, device, out=A)[1]


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_the_host_call_refuses_taps_that_are_not_finite(grid, bad):
    hist, taps = np.ones((2, 8, 2), np.uint64), np.ones((2, 3))
    taps[1, 2] = bad
    with pytest.raises(H.HareError) as ei:
        grid.hist_render(hist, taps, 4, 20)
    assert ei.value.code == capi.HARE_E_INVALID and "hare_hist_render: taps[5]" in str(ei.value)


def test_the_python_mirror_checks_shapes():
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    with pytest.raises(ValueError):
        g.hist_render(np.ones((2, 8, 2, 3), np.uint64), np.ones((2, 3)), 4, 20)
    with pytest.raises(ValueError):
        g.hist_render(np.ones((2, 8, 2), np.uint64), np.ones((3, 3)), 4, 20)
    with pytest.raises(ValueError):
        g.hist_render(np.ones((2, 8, 2), np.uint64), np.ones((2, 3)), 4, 20, weight=np.ones((8, 3), np.uint32))


@pytest.mark.skipif(H.device_count() > 0, reason="a GPU is present")
def test_without_a_device_the_calls_answer_nodevice_after_the_checks(grid):
    for device in (False, True):
        rc, msg = call(grid, device)
        assert rc == capi.HARE_E_NODEVICE, (rc, msg)
        rc, _ = call(grid, device, M=0)                                      # INVALID comes first
        assert rc == capi.HARE_E_INVALID
    with pytest.raises(H.HareError) as ei:
        grid.hist_render(np.ones((2, 8, 2), np.uint64), np.ones((2, 3)), 4, 20, seed=-1)
    assert ei.value.code == capi.HARE_E_NODEVICE
    with pytest.raises(H.HareError) as ei:
        grid.hist_render_device(2, 8, 2, 1, A, 20, 4, 3, A + (1 << 17), 7, A + (1 << 18))
    assert ei.value.code == capi.HARE_E_NODEVICE
