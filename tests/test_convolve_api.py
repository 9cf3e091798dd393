"""The convolution (include/hare_hip.h, "receivers", "Convolution") without a GPU: the two exports are bound and declared; every refusal of
the header is HARE_E_INVALID with a message that names the call, from the host call and from the device call, in the header's order;
the work cap is the header's HARE_CONVOLVE_MAX_TERMS to the term; behind the checks a GPU-less host answers HARE_E_NODEVICE; and the
Python wrapper checks its shapes."""
import re

import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi

NEW = ("hare_convolve_device", "hare_convolve")
HEADER = open(capi.os.path.join(capi.os.path.dirname(capi._HERE), "include", "hare_hip.h")).read()
CAP = 1 << int(re.search(r"#define HARE_CONVOLVE_MAX_TERMS \(\(int64_t\)1 << (\d+)\)", HEADER).group(1))


@pytest.fixture(scope="module")
def grid():
    m = H.scenes.shoebox()
    return H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)


def test_new_symbols_are_exported_bound_and_declared():
    for name in NEW:
        assert name in capi.SYMBOLS, name
        assert getattr(capi.lib, name).argtypes == capi.SYMBOLS[name][1]
        assert f"HARE_API int {name}(" in HEADER, name
    assert "Convolution (hare_convolve_device, hare_convolve)" in HEADER
    assert HEADER.index("Rendering (hare_hist_render_device") < HEADER.index("Convolution (hare_convolve_device")
    assert 1 << 36 <= CAP <= 1 << 50


# a call that passes its checks goes on to the device: such probes point at host memory, or at nothing, and run only where there is none
no_device = pytest.mark.skipif(H.device_count() > 0, reason="a GPU is present")
BUF = np.zeros(1 << 16, np.uint64)                   # 512 KiB the calls may point into: nothing is dereferenced before the checks pass
A = BUF.ctypes.data


def call(g, device, R=2, N=16, L=8, n0=0, n_out=23, ir=A, x=A + (1 << 17), y=A + (1 << 18)):
    """Either call with every argument replaceable: (rc, message).  The good arguments: ir 256 bytes at A, x 64 bytes at A + 128 KiB,
    y 368 bytes at A + 256 KiB."""
    if device:
        rc = capi.lib.hare_convolve_device(g._h, R, N, ir, L, x, n0, n_out, y, None)
    else:
        rc = capi.lib.hare_convolve(g._h, R, N, ir, L, x, n0, n_out, y)
    return rc, capi.last_error()


BIG = dict(ir=1 << 40, x=1 << 50, y=1 << 52)          # addresses far apart for shapes no buffer of the test could hold: never dereferenced
REFUSED = [dict(R=0), dict(R=-1), dict(R=(1 << 20) + 1), dict(N=0), dict(N=-5), dict(N=(1 << 24) + 1), dict(L=0), dict(L=-1), dict(L=(1 << 28) + 1),
           dict(n0=-1), dict(n_out=0), dict(n_out=-3), dict(n_out=24), dict(n0=1), dict(n0=23, n_out=1), dict(n0=1 << 62, n_out=1 << 62),
           dict(R=1 << 20, N=1 << 8, L=1 << 8, n_out=257, **BIG),                          # R x n_out = 2^28 + 2^20
           dict(R=1 << 10, N=1 << 20, L=1 << 24, n_out=(1 << 18) + 1, **BIG),
           dict(R=1 << 10, N=1 << 24, L=1 << 24, n_out=1 << 18, **BIG),                    # 2^52 terms: above any cap
           dict(R=1, N=1 << 24, L=1 << 28, n_out=(CAP >> 24) + 1, **BIG),
           dict(ir=None), dict(x=None), dict(y=None),
           dict(y=A), dict(y=A + 248), dict(y=A - 360), dict(y=A + (1 << 17)), dict(y=A + (1 << 17) + 56), dict(y=A + (1 << 17) - 360)]


def case_id(kw):
    """A pointer into BUF is named by its offset from A: the address differs from process to process, a test's name must not"""
    return ",".join(f"{k}=A+{v - A}" if k in ("ir", "x", "y") and v is not None and v >= A - 4096 and v < A + (1 << 20) else f"{k}={v}" for k, v in kw.items())[:70]


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("kw", REFUSED, ids=case_id)
def test_every_refusal_is_invalid_and_names_the_call(grid, kw, device):
    rc, msg = call(grid, device, **kw)
    assert rc == capi.HARE_E_INVALID, (kw, rc, msg)
    assert msg.startswith("hare_convolve_device:" if device else "hare_convolve:"), msg


def test_a_null_scene_is_refused():
    assert capi.lib.hare_convolve(None, 2, 16, A, 8, A + (1 << 17), 0, 23, A + (1 << 18)) == capi.HARE_E_INVALID
    assert capi.lib.hare_convolve_device(None, 2, 16, A, 8, A + (1 << 17), 0, 23, A + (1 << 18), None) == capi.HARE_E_INVALID


def test_the_checks_come_in_the_headers_order(grid):
    over_out = dict(R=1 << 20, N=1 << 8, L=1 << 8, n_out=257)
    over_work = dict(R=1 << 10, N=1 << 24, L=1 << 24, n_out=1 << 18)
    for device in (False, True):
        assert "R out of range" in call(grid, device, R=0, N=0, L=0, n_out=0, ir=None)[1]
        assert "N out of range" in call(grid, device, N=0, L=0, n_out=0, ir=None)[1]
        assert "L out of range" in call(grid, device, L=0, n_out=0, ir=None)[1]
        assert "window" in call(grid, device, n_out=0, ir=None)[1]
        assert "window" in call(grid, device, **dict(over_out, n_out=1 << 10), ir=None)[1]
        assert "2^28" in call(grid, device, **over_out, ir=None)[1]
        assert "work cap" in call(grid, device, **over_work, ir=None)[1]
        assert "null" in call(grid, device, ir=None, y=A)[1]
        assert "overlap" in call(grid, device, y=A)[1]


@no_device
def test_the_overlap_check_is_to_the_byte(grid):
    """y (368 bytes) may touch ir (256 bytes at A) and x (64 bytes at A + 128 KiB) but share no byte with them"""
    for device in (False, True):
        for y in (A + 255, A - 367, A + (1 << 17) + 63, A + (1 << 17) - 367):
            assert call(grid, device, y=y)[0] == capi.HARE_E_INVALID, y - A
        for y in (A + 256, A - 368, A + (1 << 17) + 64, A + (1 << 17) - 368):
            assert call(grid, device, y=y)[0] != capi.HARE_E_INVALID, y - A
        assert call(grid, device, x=A + 8)[0] != capi.HARE_E_INVALID          # the two inputs may overlap each other


@no_device
def test_the_work_cap_is_the_headers_to_the_term(grid):
    """R = 1, N = 2^24 <= L: the bound is n_out x 2^24"""
    n = CAP >> 24                                                          # < 2^28: the output cap does not come first
    for device in (False, True):
        rc, msg = call(grid, device, R=1, N=1 << 24, L=1 << 28, n_out=n, **BIG)
        assert rc != capi.HARE_E_INVALID, msg
        rc, msg = call(grid, device, R=1, N=1 << 24, L=1 << 28, n_out=n + 1, **BIG)
        assert rc == capi.HARE_E_INVALID and "work cap" in msg


def test_the_python_wrapper_checks_shapes(grid):
    for ir, x in ((np.ones(5), np.ones(3)), (np.ones((2, 2, 2, 5)), np.ones(3)), (np.ones((2, 5)), np.ones((1, 3))), (np.ones((2, 0)), np.ones(3)),
                  (np.ones((2, 5)), np.ones(0))):
        with pytest.raises(ValueError):
            grid.convolve(ir, x)
    for kw in (dict(n0=7), dict(n0=-1), dict(n0=0, n_out=8), dict(n0=3, n_out=0)):          # N + L - 1 = 7
        with pytest.raises(H.HareError) as ei:
            grid.convolve(np.ones((2, 5)), np.ones(3), **kw)
        assert ei.value.code == capi.HARE_E_INVALID and "window" in str(ei.value)


@no_device
def test_without_a_device_the_calls_answer_nodevice_after_the_checks(grid):
    for device in (False, True):
        rc, msg = call(grid, device)
        assert rc == capi.HARE_E_NODEVICE, (rc, msg)
        rc, _ = call(grid, device, n_out=0)                                  # INVALID comes first
        assert rc == capi.HARE_E_INVALID
    with pytest.raises(H.HareError) as ei:
        grid.convolve(np.ones((2, 4, 5)), np.ones(3))                        # [K, C, N] is flattened to rows
    assert ei.value.code == capi.HARE_E_NODEVICE
    with pytest.raises(H.HareError) as ei:
        grid.convolve_device(2, 16, A, 8, A + (1 << 17), 0, 23, A + (1 << 18))
    assert ei.value.code == capi.HARE_E_NODEVICE
