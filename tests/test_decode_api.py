"""The decoding (include/hare_hip.h, "receivers", "Decoding") without a GPU: the two exports are bound and declared; every refusal of the
header is HARE_E_INVALID with a message that names the call, from the host call and from the device call, in the header's order; the
work cap is the header's HARE_DECODE_MAX_TERMS to the term, a constant of its own that capi repeats; behind the checks a GPU-less host
answers HARE_E_NODEVICE; and the Python wrapper checks its shapes."""
import re

import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi

NEW = ("hare_decode_device", "hare_decode")
HEADER = open(capi.os.path.join(capi.os.path.dirname(capi._HERE), "include", "hare_hip.h")).read()
CAP = 1 << int(re.search(r"#define HARE_DECODE_MAX_TERMS \(\(int64_t\)1 << (\d+)\)", HEADER).group(1))


@pytest.fixture(scope="module")
def grid():
    m = H.scenes.shoebox()
    return H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)


def test_new_symbols_are_exported_bound_and_declared():
    for name in NEW:
        assert name in capi.SYMBOLS, name
        assert getattr(capi.lib, name).argtypes == capi.SYMBOLS[name][1]
        assert f"HARE_API int {name}(" in HEADER, name
    assert "Decoding (hare_decode_device, hare_decode)" in HEADER
    assert HEADER.index("Convolution (hare_convolve_device") < HEADER.index("Decoding (hare_decode_device") < HEADER.index("Setters: single-caller")
    assert capi.DECODE_MAX_TERMS == CAP and 1 << 36 <= CAP < 1 << 50
    assert 'a decode matrix is another call\'s\n * business: "Decoding" below' in HEADER          # the convolution's sentence has its pointer
    assert "IS hare_convolve with ir = h" in HEADER


# a call that passes its checks goes on to the device: such probes point at host memory, or at nothing, and run only where there is none
no_device = pytest.mark.skipif(H.device_count() > 0, reason="a GPU is present")
BUF = np.zeros(1 << 16, np.uint64)                   # 512 KiB the calls may point into: nothing is dereferenced before the checks pass
A = BUF.ctypes.data


def call(g, device, K=2, C=3, N=16, O=2, T=8, n0=0, n_out=23, x=A, h=A + (1 << 17), y=A + (1 << 18)):
    """Either call with every argument replaceable: (rc, message).  The good arguments: in 768 bytes at A, h 384 bytes at A + 128 KiB,
    y 736 bytes at A + 256 KiB."""
    if device:
        rc = capi.lib.hare_decode_device(g._h, K, C, N, x, O, T, h, n0, n_out, y, None)
    else:
        rc = capi.lib.hare_decode(g._h, K, C, N, x, O, T, h, n0, n_out, y)
    return rc, capi.last_error()


BIG = dict(x=1 << 40, h=1 << 50, y=1 << 52)          # addresses far apart for shapes no buffer of the test could hold: never dereferenced
OVER_IN = dict(K=1 << 16, C=64, N=(1 << 6) + 1, O=1, T=1, n_out=1)                     # K x C x N = 2^28 + 2^22
OVER_OUT = dict(K=1 << 16, C=1, N=1 << 12, O=64, T=1 << 8, n_out=(1 << 6) + 1)         # K x O x n_out = 2^28 + 2^22
OVER_WORK = dict(K=1, C=64, N=1 << 22, O=64, T=1 << 16, n_out=1 << 22)                 # 2^28 outputs x 2^6 x 2^16 = 2^50 terms: above any cap
REFUSED = [dict(K=0), dict(K=-1), dict(K=(1 << 16) + 1), dict(C=0), dict(C=-2), dict(C=65), dict(O=0), dict(O=-1), dict(O=65),
           dict(N=0), dict(N=-5), dict(N=(1 << 24) + 1), dict(T=0), dict(T=-1), dict(T=(1 << 16) + 1),
           dict(n0=-1), dict(n_out=0), dict(n_out=-3), dict(n_out=24), dict(n0=1), dict(n0=23, n_out=1), dict(n0=1 << 62, n_out=1 << 62),
           dict(OVER_IN, **BIG), dict(OVER_OUT, **BIG), dict(OVER_WORK, **BIG),
           dict(K=64, C=64, N=1 << 16, O=64, T=1 << 16, n_out=(CAP >> 34) + 1, **BIG),     # one output over the cap
           dict(x=None), dict(h=None), dict(y=None),
           dict(y=A), dict(y=A + 760), dict(y=A - 728), dict(y=A + (1 << 17)), dict(y=A + (1 << 17) + 376), dict(y=A + (1 << 17) - 728)]


def case_id(kw):
    """A pointer into BUF is named by its offset from A: the address differs from process to process, a test's name must not"""
    return ",".join(f"{k}=A+{v - A}" if k in ("x", "h", "y") and v is not None and v >= A - 4096 and v < A + (1 << 20) else f"{k}={v}" for k, v in kw.items())[:70]


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("kw", REFUSED, ids=case_id)
def test_every_refusal_is_invalid_and_names_the_call(grid, kw, device):
    rc, msg = call(grid, device, **kw)
    assert rc == capi.HARE_E_INVALID, (kw, rc, msg)
    assert msg.startswith("hare_decode_device:" if device else "hare_decode:"), msg


def test_a_null_scene_is_refused():
    assert capi.lib.hare_decode(None, 2, 3, 16, A, 2, 8, A + (1 << 17), 0, 23, A + (1 << 18)) == capi.HARE_E_INVALID
    assert capi.lib.hare_decode_device(None, 2, 3, 16, A, 2, 8, A + (1 << 17), 0, 23, A + (1 << 18), None) == capi.HARE_E_INVALID


def test_the_checks_come_in_the_headers_order(grid):
    for device in (False, True):
        assert "K out of range" in call(grid, device, K=0, C=0, O=0, N=0, T=0, n_out=0, x=None)[1]
        assert "C out of range" in call(grid, device, C=0, O=0, N=0, T=0, n_out=0, x=None)[1]
        assert "O out of range" in call(grid, device, O=0, N=0, T=0, n_out=0, x=None)[1]
        assert "N out of range" in call(grid, device, N=0, T=0, n_out=0, x=None)[1]
        assert "T out of range" in call(grid, device, T=0, n_out=0, x=None)[1]
        assert "window" in call(grid, device, n_out=0, x=None)[1]
        assert "window" in call(grid, device, **dict(OVER_IN, n_out=1 << 10), x=None)[1]
        assert "K x C x N exceeds 2^28" in call(grid, device, **dict(OVER_IN, O=64, n_out=(1 << 6) + 1), x=None)[1]          # the outputs are over too
        assert "K x O x n_out exceeds 2^28" in call(grid, device, **OVER_OUT, x=None)[1]
        assert "work cap" in call(grid, device, **OVER_WORK, x=None)[1]
        assert "null" in call(grid, device, x=None, y=A)[1]
        assert "overlap" in call(grid, device, y=A)[1]


@no_device
def test_the_overlap_check_is_to_the_byte(grid):
    """y (736 bytes) may touch in (768 bytes at A) and h (384 bytes at A + 128 KiB) but share no byte with them"""
    for device in (False, True):
        for y in (A + 767, A - 735, A + (1 << 17) + 383, A + (1 << 17) - 735):
            assert call(grid, device, y=y)[0] == capi.HARE_E_INVALID, y - A
        for y in (A + 768, A - 736, A + (1 << 17) + 384, A + (1 << 17) - 736):
            assert call(grid, device, y=y)[0] != capi.HARE_E_INVALID, y - A
        assert call(grid, device, h=A + 8)[0] != capi.HARE_E_INVALID          # the two inputs may overlap each other


@no_device
def test_the_work_cap_is_the_headers_to_the_term(grid):
    """K = 64, O = 64, C = 64, N = T = 2^16, so min(N, T) = 2^16 and n_out <= 2^16: the bound is n_out x 2^34"""
    n = CAP >> 34
    assert 1 <= n < 1 << 16                                                # the output cap (2^28 = 2^12 x 2^16) does not come first
    kw = dict(K=64, C=64, N=1 << 16, O=64, T=1 << 16, **BIG)
    for device in (False, True):
        rc, msg = call(grid, device, n_out=n, **kw)
        assert rc != capi.HARE_E_INVALID, msg
        rc, msg = call(grid, device, n_out=n + 1, **kw)
        assert rc == capi.HARE_E_INVALID and "work cap" in msg


def test_the_python_wrapper_checks_shapes(grid):
    ok_x, ok_h = np.ones((2, 3, 5)), np.ones((2, 3, 4))
    for x, h in ((np.ones((3, 5)), ok_h), (np.ones((2, 2, 3, 5)), ok_h), (ok_x, np.ones((3, 4))), (ok_x, np.ones((2, 4, 4))), (np.ones((2, 3, 0)), ok_h),
                 (ok_x, np.ones((0, 3, 4))), (ok_x, np.ones(4))):
        with pytest.raises(ValueError):
            grid.decode(x, h)
    for kw in (dict(n0=8), dict(n0=-1), dict(n0=0, n_out=9), dict(n0=3, n_out=0)):          # N + T - 1 = 8
        with pytest.raises(H.HareError) as ei:
            grid.decode(ok_x, ok_h, **kw)
        assert ei.value.code == capi.HARE_E_INVALID and "window" in str(ei.value)


@no_device
def test_without_a_device_the_calls_answer_nodevice_after_the_checks(grid):
    for device in (False, True):
        rc, msg = call(grid, device)
        assert rc == capi.HARE_E_NODEVICE, (rc, msg)
        rc, _ = call(grid, device, n_out=0)                                  # INVALID comes first
        assert rc == capi.HARE_E_INVALID
    with pytest.raises(H.HareError) as ei:
        grid.decode(np.ones((2, 4, 5)), np.ones((2, 4, 3)))
    assert ei.value.code == capi.HARE_E_NODEVICE
    with pytest.raises(H.HareError) as ei:
        grid.decode_device(2, 3, 16, A, 2, 8, A + (1 << 17), 0, 23, A + (1 << 18))
    assert ei.value.code == capi.HARE_E_NODEVICE
