"""The impulses (include/hare_hip.h, "receivers", "Impulses") without a GPU: the three exports are bound and declared; every refusal of
the header is HARE_E_INVALID with a message that names the call, from the host call and from the device call, in the header's order; the
host call also refuses a tap that is not finite; hare_source_paths keeps its flag rules; behind the checks a GPU-less host answers
HARE_E_NODEVICE; and the Python wrappers check their shapes."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi

NEW = ("hare_hist_impulses_device", "hare_hist_impulses", "hare_source_paths")
HEADER = open(capi.os.path.join(capi.os.path.dirname(capi._HERE), "include", "hare_hip.h")).read()


@pytest.fixture(scope="module")
def grid():
    m = H.scenes.shoebox()
    return H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)


def test_new_symbols_are_exported_bound_and_declared():
    for name in NEW:
        assert name in capi.SYMBOLS, name
        assert getattr(capi.lib, name).argtypes == capi.SYMBOLS[name][1]
        assert f"HARE_API int {name}(" in HEADER, name
    assert "Impulses (hare_hist_impulses_device, hare_hist_impulses, hare_source_paths)" in HEADER
    assert HEADER.index("Rendering (hare_hist_render_device") < HEADER.index("Impulses (hare_hist_impulses_device") < HEADER.index("Convolution (hare_convolve_device")
    assert H.unit_energy_taps is H.geometry.unit_energy_taps and "unit_energy_taps" in H.__all__


no_device = pytest.mark.skipif(H.device_count() > 0, reason="a GPU is present")
BUF = np.zeros(1 << 16, np.uint64)                   # 512 KiB the calls may point into: nothing is dereferenced before the checks pass
BUF[1 << 14:] = 0x3FF0000000000000                   # ... but the host call reads its taps (at A + 128 KiB): 1.0 each
A = BUF.ctypes.data
TAPS, OUT, WEIGHT = A + (1 << 17), A + (1 << 18), A + (1 << 16)


def call(g, device, K=2, n_bins=16, B=3, C=4, hist=A, weight=None, frac_bits=24, T=8, taps=TAPS, n0=0, n_out=23, stride=None, add=0, out=OUT):
    """Either call with every argument replaceable: (rc, message).  The good arguments: the histogram 3 072 bytes at A, the taps 192 bytes at
    A + 128 KiB, out 1 472 bytes at A + 256 KiB"""
    stride = n_out if stride is None else stride
    if device:
        rc = capi.lib.hare_hist_impulses_device(g._h, K, n_bins, B, C, hist, weight, frac_bits, T, taps, n0, n_out, stride, add, out, None)
    else:
        rc = capi.lib.hare_hist_impulses(g._h, K, n_bins, B, C, hist, weight, frac_bits, T, taps, n0, n_out, stride, add, out)
    return rc, capi.last_error()


BIG = dict(hist=1 << 40, taps=TAPS, out=1 << 52)
REFUSED = [dict(K=0), dict(K=-1), dict(K=(1 << 16) + 1), dict(n_bins=0), dict(n_bins=-4), dict(B=0), dict(B=9), dict(C=0), dict(C=2), dict(C=3), dict(C=17),
           dict(K=1 << 16, n_bins=(1 << 7) + 1, B=1, C=16, n_out=1, **BIG),          # 2^27 + 2^20 words
           dict(T=0), dict(T=-1), dict(T=1025), dict(frac_bits=-1), dict(frac_bits=63),
           dict(n0=-1), dict(n_out=0), dict(n_out=-3), dict(n_out=24), dict(n0=1), dict(n0=23, n_out=1), dict(n0=1 << 62, n_out=1 << 62),
           dict(stride=22), dict(stride=0), dict(stride=-1),
           dict(K=1 << 12, C=16, n_bins=1 << 8, B=1, T=1, n_out=1, stride=(1 << 12) + 1, **BIG),          # K x channels x out_stride = 2^28 + 2^16
           dict(stride=1 << 62),
           dict(add=2), dict(add=-1),
           dict(hist=None), dict(taps=None), dict(out=None),
           dict(out=A), dict(out=A + 3064), dict(out=A - 1464), dict(out=TAPS), dict(out=TAPS + 184), dict(out=TAPS - 1464),
           dict(weight=WEIGHT, out=WEIGHT), dict(weight=WEIGHT, out=WEIGHT + 184), dict(weight=WEIGHT, out=WEIGHT - 1464)]


def case_id(kw):
    names = {A: "A", TAPS: "TAPS", WEIGHT: "WEIGHT", OUT: "OUT"}
    def show(k, v):
        if k in ("hist", "taps", "out", "weight") and v is not None and A - 4096 <= v < A + (1 << 20):
            base = max(b for b in names if b <= max(v, A))
            return f"{k}={names[base]}{v - base:+d}"
        return f"{k}={v}"
    return ",".join(show(k, v) for k, v in kw.items())[:70]


@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("kw", REFUSED, ids=case_id)
def test_every_refusal_is_invalid_and_names_the_call(grid, kw, device):
    rc, msg = call(grid, device, **kw)
    assert rc == capi.HARE_E_INVALID, (kw, rc, msg)
    assert msg.startswith("hare_hist_impulses_device:" if device else "hare_hist_impulses:"), msg


def test_a_null_scene_is_refused():
    assert capi.lib.hare_hist_impulses(None, 2, 16, 3, 4, A, None, 24, 8, TAPS, 0, 23, 23, 0, OUT) == capi.HARE_E_INVALID
    assert capi.lib.hare_hist_impulses_device(None, 2, 16, 3, 4, A, None, 24, 8, TAPS, 0, 23, 23, 0, OUT, None) == capi.HARE_E_INVALID
    assert capi.lib.hare_source_paths(None, capi.KIND_VOXEL, 0, 1, capi.RECEIVE_DIRECT, 16, 1.0, 24, A, OUT) == capi.HARE_E_INVALID


def test_the_checks_come_in_the_headers_order(grid):
    worse = dict(T=0, frac_bits=-1, n_out=0, stride=-1, add=2, hist=None)
    for device in (False, True):
        assert "K out of range" in call(grid, device, K=0, n_bins=0, B=0, C=0, **worse)[1]
        assert "n_bins" in call(grid, device, n_bins=0, B=0, C=0, **worse)[1]
        assert "bands out of range" in call(grid, device, B=0, C=0, **worse)[1]
        assert "channels" in call(grid, device, C=0, **worse)[1]
        assert "2^27" in call(grid, device, K=1 << 16, n_bins=(1 << 7) + 1, B=1, C=16, **worse)[1]
        assert "T out of range" in call(grid, device, **worse)[1]
        assert "frac_bits" in call(grid, device, **dict(worse, T=8))[1]
        assert "window" in call(grid, device, **dict(worse, T=8, frac_bits=0))[1]
        assert "out_stride" in call(grid, device, stride=22, add=2, hist=None)[1]
        assert "2^28" in call(grid, device, K=1 << 12, C=16, n_bins=1 << 8, B=1, T=1, n_out=1, stride=(1 << 12) + 1, add=2, hist=None)[1]
        assert "add must be" in call(grid, device, add=2, hist=None)[1]
        assert "null" in call(grid, device, hist=None, out=A)[1]
        assert "overlap" in call(grid, device, out=A)[1]
    rc, msg = call(grid, False, taps=A)                # the host call alone reads the taps: 0.0 each at A, and one NaN put there
    assert rc != capi.HARE_E_INVALID, msg
    BUF[5] = 0x7FF8000000000000
    try:
        rc, msg = call(grid, False, taps=A, hist=A + 4096)
        assert rc == capi.HARE_E_INVALID and "taps[5] is not finite" in msg
        assert "overlap" in call(grid, False, taps=A, hist=A + 4096, out=A)[1]          # the buffers' checks come first
        assert call(grid, True, taps=A, hist=A + 4096)[0] != capi.HARE_E_INVALID          # the device call cannot look
    finally:
        BUF[5] = 0


@no_device
def test_the_overlap_check_is_to_the_byte(grid):
    """out (1 472 bytes) may touch the histogram (3 072 bytes at A), the taps (192 bytes) and the weights (192 bytes) but share no byte"""
    for device in (False, True):
        for out in (A + 3071, A - 1471, TAPS + 191, TAPS - 1471):
            assert call(grid, device, out=out)[0] == capi.HARE_E_INVALID, out - A
        for out in (A + 3072, A - 1472, TAPS + 192, TAPS - 1472):
            assert call(grid, device, out=out)[0] != capi.HARE_E_INVALID, out - A
        assert call(grid, device, weight=WEIGHT, out=WEIGHT + 191)[0] == capi.HARE_E_INVALID
        assert call(grid, device, weight=WEIGHT, out=WEIGHT + 192)[0] != capi.HARE_E_INVALID
        assert call(grid, device, out=WEIGHT + 8)[0] != capi.HARE_E_INVALID          # no weights given: nothing there to overlap
        assert call(grid, device, stride=40, out=A - 8 * 2 * 4 * 40)[0] != capi.HARE_E_INVALID          # the rows' extent is K x channels x out_stride
        assert call(grid, device, stride=40, out=A - 8 * 2 * 4 * 40 + 1)[0] == capi.HARE_E_INVALID


@no_device
def test_without_a_device_the_calls_answer_nodevice_after_the_checks(grid):
    for device in (False, True):
        rc, msg = call(grid, device)
        assert rc == capi.HARE_E_NODEVICE, (rc, msg)
        assert call(grid, device, n0=22, n_out=1, stride=5, add=1)[0] == capi.HARE_E_NODEVICE
        assert call(grid, device, n_out=0)[0] == capi.HARE_E_INVALID          # INVALID comes first
    with pytest.raises(H.HareError) as ei:
        grid.hist_impulses(np.ones((2, 5, 3, 4), np.uint64), np.ones((3, 7)), 24)
    assert ei.value.code == capi.HARE_E_NODEVICE
    with pytest.raises(H.HareError) as ei:
        grid.hist_impulses_device(2, 16, 3, 4, A, 24, 8, TAPS, 0, 23, 23, 0, OUT)
    assert ei.value.code == capi.HARE_E_NODEVICE


def test_the_python_wrapper_checks_shapes(grid):
    hist = np.ones((2, 5, 3, 4), np.uint64)
    for taps in (np.ones((2, 7)), np.ones(7), np.ones((3, 0))):
        with pytest.raises(ValueError):
            grid.hist_impulses(hist, taps, 24)
    for out in (np.zeros((2, 4, 11), np.float32), np.zeros((2, 3, 11)), np.zeros((2, 4, 22))[..., ::2], np.zeros((8, 11))):
        with pytest.raises(ValueError):
            grid.hist_impulses(hist, np.ones((3, 7)), 24, out=out)
    for kw in (dict(n0=11), dict(n0=-1), dict(n0=0, n_out=12), dict(n0=3, n_out=0), dict(out=np.zeros((2, 4, 10)))):          # n_bins + T - 1 = 11
        with pytest.raises(H.HareError) as ei:
            grid.hist_impulses(hist, np.ones((3, 7)), 24, **kw)
        assert ei.value.code == capi.HARE_E_INVALID
    t = H.unit_energy_taps([[3.0, 4.0], [0.0, 0.0], [-2.0, 0.0]])
    assert t.tolist() == [[0.6, 0.8], [0.0, 0.0], [-1.0, 0.0]]
    with pytest.raises(ValueError):
        H.unit_energy_taps([[1.0, np.inf]])


# ---- hare_source_paths
def paths(g, flags, kind=None, top=0, n_weight=4097, n_bins=64, bin_len=0.5, frac_bits=40, hist=A, det=OUT):
    rc = capi.lib.hare_source_paths(g._h, g._kind if kind is None else kind, top, n_weight, flags, n_bins, bin_len, frac_bits, hist, det)
    return rc, capi.last_error()


@pytest.fixture(scope="module")
def room():
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.set_receivers(np.array([[3.0, 2.0, 1.5], [6.0, 4.0, 2.0]]), np.array([0.25, 0.5]))
    g.set_source((2.0, 1.0, 1.0))
    return g


D, I, I2 = capi.RECEIVE_DIRECT, capi.RECEIVE_IMAGE, capi.RECEIVE_IMAGE2
DIR, O2, O3 = capi.RECEIVE_DIRECTIONAL, capi.RECEIVE_ORDER2, capi.RECEIVE_ORDER3


def test_source_paths_flag_rules(room):
    for flags in (0, DIR, DIR | O3, I2, D | I2, D | capi.RECEIVE_DIFFUSE_RAIN, D | capi.RECEIVE_TIME_LIMIT, D | 1, D | (1 << 30), D | O2, D | O3,
                  D | DIR | O2 | O3):
        rc, msg = paths(room, flags)
        assert rc == capi.HARE_E_INVALID and msg.startswith("hare_source_paths:"), (flags, rc, msg)
    assert "nothing to deposit" in paths(room, DIR)[1] and "HARE_RECEIVE_IMAGE2 is accepted only together" in paths(room, I2 | D)[1]
    assert "flags other than" in paths(room, D | capi.RECEIVE_TIME_LIMIT)[1]
    for flags in (D, I, I | I2, D | I, D | I | I2, D | DIR, I | I2 | DIR | O2, D | I | I2 | DIR | O3):
        rc, msg = paths(room, flags)
        assert rc != capi.HARE_E_INVALID, (flags, msg)


def test_source_paths_refusals(room):
    ok = D | I | I2
    for kw in (dict(kind=7), dict(top=1), dict(top=-1), dict(n_weight=0), dict(n_weight=(1 << 53) + 1), dict(n_bins=0), dict(bin_len=0.0),
               dict(bin_len=float("nan")), dict(frac_bits=63), dict(frac_bits=-1), dict(hist=None), dict(det=None), dict(det=A), dict(det=A + 8 * 2 * 64 - 1),
               dict(n_bins=(1 << 27) // 2 + 1)):
        rc, msg = paths(room, ok, **kw)
        assert rc == capi.HARE_E_INVALID and msg.startswith("hare_source_paths:"), (kw, rc, msg)
    assert paths(room, ok, det=A + 8 * 2 * 64)[0] != capi.HARE_E_INVALID          # K x n_bins x B words of histogram, then the detections may begin
    assert paths(room, ok | DIR, det=A + 8 * 2 * 64)[0] == capi.HARE_E_INVALID     # four channels: the histogram is four times as long


@no_device
def test_source_paths_without_a_device(room, grid):
    assert paths(room, D | I | I2)[0] == capi.HARE_E_NODEVICE
    assert paths(grid, D)[0] == capi.HARE_E_NODEVICE          # no source, no receivers: HARE_E_STATE is the device's to say
    with pytest.raises(H.HareError) as ei:
        room.Source_paths(4097, 2048, 343.0 / 48000)
    assert ei.value.code == capi.HARE_E_NODEVICE
    with pytest.raises(H.HareError) as ei:
        room.Source_paths(4097, 64, 0.5, image=False)           # image2 alone
    assert ei.value.code == capi.HARE_E_INVALID
    with pytest.raises(ValueError):
        room.Source_paths(4097, 64, 0.5, directional=True, order=4)
