"""The reduction of a histogram (include/hare_hip.h, "receivers", "Reduction") without a GPU: the four exports are bound and declared;
every refusal of the header is HARE_E_INVALID with a message that names the call; behind the checks a GPU-less host answers
HARE_E_NODEVICE; air_weights and decay_levels at hand-computed points; and the restatement's own sanity (tests/reduce_ref.py): its two
forms agree, the crossings of an exponential decay lie within a bin of the closed form, S1 / S0 of a single bin is that bin."""
import math

import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests.reduce_ref import reduce_direct, reduce_ref

NEW = ("hare_hist_reduce_device", "hare_hist_reduce", "hare_receive_batch_reduced", "hare_receive_source_reduced")


@pytest.fixture(scope="module")
def grid():
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.set_receivers([[1.0, 1.0, 1.0], [2.0, 1.0, 1.0]], [0.3, 0.3])
    g.set_source([1.5, 1.5, 1.0])
    return g


def test_new_symbols_are_exported_bound_and_declared():
    hdr = open(capi.os.path.join(capi.os.path.dirname(capi._HERE), "include", "hare_hip.h")).read()
    for name in NEW:
        assert name in capi.SYMBOLS, name
        assert getattr(capi.lib, name).argtypes == capi.SYMBOLS[name][1]
        assert f"HARE_API int {name}(" in hdr, name


def host_call(g, K=2, n_bins=8, B=1, channels=1, hist=True, weight=None, win=((0, 8),), levels=(1 << 31,), sums=True, cross=True, alias=None):
    """hare_hist_reduce with every argument replaceable: (rc, message)."""
    words = max(1, K * n_bins * B * channels) if 0 < K * n_bins * B * channels <= 1 << 20 else 1
    h = np.zeros(words, np.uint64)
    w = None if win is None else np.asarray(win, np.int32).reshape(-1)
    n_win = 0 if win is None else len(win)
    lv = None if levels is None else np.asarray(levels, np.uint32)
    n_lev = 0 if levels is None else len(levels)
    s = np.zeros(max(1, abs(K * B) * 64 * 4) if abs(K * B) < 1 << 16 else 1, np.uint64)
    c = np.zeros(max(1, abs(K * B) * 32) if abs(K * B) < 1 << 16 else 1, np.int32)
    ps, pc = capi.ptr(s) if sums else None, capi.ptr(c) if cross else None
    if alias == "sums=hist":
        ps = capi.ptr(h)
    if alias == "cross=sums":
        pc = ps
    if alias == "cross=weight":
        pc = capi.ptr(weight)
    rc = capi.lib.hare_hist_reduce(g._h, K, n_bins, B, channels, capi.ptr(h) if hist else None, capi.ptr(weight), n_win, capi.ptr(w), n_lev,
                                   capi.ptr(lv), ps, pc)
    return rc, capi.last_error()


REFUSED = [dict(K=0), dict(K=65537), dict(n_bins=0), dict(n_bins=-1), dict(B=0), dict(B=9), dict(K=65536, n_bins=1025, B=2),
           dict(K=4096, n_bins=4096, B=2, channels=4), dict(channels=0), dict(channels=2), dict(channels=3), dict(channels=5),
           dict(win=((0, 1),) * 17), dict(levels=(1,) * 33), dict(win=None, levels=None), dict(win=((3, 2),)), dict(win=((-1, 2),)),
           dict(win=((0, 9),)), dict(win=((0, 8), (9, 9))), dict(hist=False), dict(sums=False), dict(cross=False), dict(alias="sums=hist"),
           dict(alias="cross=sums"), dict(alias="cross=weight", weight=np.ones(8, np.uint32))]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: ",".join(f"{k}={'...' if isinstance(v, np.ndarray) else v}" for k, v in kw.items())[:60])
def test_every_refusal_is_invalid_and_names_the_call(grid, kw):
    rc, msg = host_call(grid, **kw)
    assert rc == capi.HARE_E_INVALID, (kw, rc, msg)
    assert msg.startswith("hare_hist_reduce:"), msg


def test_counts_out_of_range_and_null_arrays_are_refused(grid):
    h, s, c = np.zeros(16, np.uint64), np.zeros(4096, np.uint64), np.zeros(4096, np.int32)
    w, lv = np.zeros(64, np.int32), np.zeros(64, np.uint32)
    for n_win, pw, n_lev, pl in ((-1, w, 1, lv), (17, w, 0, lv), (1, w, -1, lv), (0, w, 33, lv), (0, w, 0, lv), (1, None, 0, lv), (0, w, 1, None)):
        for dev in (False, True):
            if dev:
                rc = capi.lib.hare_hist_reduce_device(grid._h, 2, 8, 1, 1, capi.ptr(h), None, n_win, capi.ptr(pw), n_lev, capi.ptr(pl), capi.ptr(s),
                                                      capi.ptr(c), None)
            else:
                rc = capi.lib.hare_hist_reduce(grid._h, 2, 8, 1, 1, capi.ptr(h), None, n_win, capi.ptr(pw), n_lev, capi.ptr(pl), capi.ptr(s), capi.ptr(c))
            assert rc == capi.HARE_E_INVALID, (n_win, n_lev, dev)
            assert capi.last_error().startswith("hare_hist_reduce_device:" if dev else "hare_hist_reduce:")
    assert capi.lib.hare_hist_reduce(None, 2, 8, 1, 1, capi.ptr(h), None, 1, capi.ptr(w), 0, None, capi.ptr(s), None) == capi.HARE_E_INVALID


def test_the_device_call_checks_the_same_things(grid):
    one = np.zeros(4096, np.uint64)
    a = one.ctypes.data                                        # any non-null addresses: nothing is dereferenced before the checks pass
    win, lv = np.array([0, 8], np.int32), np.array([5], np.uint32)
    def call(K=2, n_bins=8, B=1, channels=1, d_hist=a, d_sums=a + 8192, d_cross=a + 16384, d_weight=None, win=win):
        return capi.lib.hare_hist_reduce_device(grid._h, K, n_bins, B, channels, d_hist, d_weight, 1, capi.ptr(win), 1, capi.ptr(lv), d_sums, d_cross, None)
    for kw in (dict(K=0), dict(n_bins=0), dict(B=9), dict(channels=2), dict(K=65536, n_bins=2049), dict(win=np.array([5, 4], np.int32)),
               dict(d_hist=None), dict(d_sums=None), dict(d_cross=None), dict(d_sums=a), dict(d_cross=a + 8192 + 8), dict(d_weight=a + 16384)):
        assert call(**kw) == capi.HARE_E_INVALID, kw
        assert capi.last_error().startswith("hare_hist_reduce_device:"), capi.last_error()


def test_the_reduced_receive_calls_check_parent_and_reduction(grid):
    rays = np.zeros((8, 6))
    rays[:, 3] = 1.0
    good = dict(windows=[(0, 4)], levels=[1 << 31])
    for kw in (dict(windows=[(0, 5)]), dict(windows=[(2, 1)]), dict(windows=[(0, 1)] * 17), dict(levels=[1] * 33), dict()):
        for source in (False, True):
            with pytest.raises(H.HareError) as ei:
                if source:
                    grid.Receive_source_reduced(8, 2, 4, 0.5, **kw)
                else:
                    grid.Receive_batch_reduced(rays, 2, 4, 0.5, **kw)
            assert ei.value.code == capi.HARE_E_INVALID, kw
            assert ("hare_receive_source_reduced:" if source else "hare_receive_batch_reduced:") in str(ei.value)
    with pytest.raises(H.HareError) as ei:                     # the parent's own checks come first
        grid.Receive_batch_reduced(rays, 0, 4, 0.5, **good)
    assert ei.value.code == capi.HARE_E_INVALID and "hare_receive_batch_reduced: bounces" in str(ei.value)
    s, c, d = np.zeros(64, np.uint64), np.zeros(64, np.int32), np.zeros(4, np.uint64)
    win, lv = np.array([0, 4], np.int32), np.array([5], np.uint32)
    for ps, pc, pd in ((None, c, d), (s, None, d), (s, c, None), (s, s.view(np.int32), d), (d, c, d)):
        rc = capi.lib.hare_receive_batch_reduced(grid._h, grid._kind, 0, 8, capi.ptr(rays), None, None, 2, 0, 4, 0.5, 30, None, None, None, 1,
                                                 capi.ptr(win), 1, capi.ptr(lv), capi.ptr(ps), capi.ptr(pc), capi.ptr(pd), None)
        assert rc == capi.HARE_E_INVALID and capi.last_error().startswith("hare_receive_batch_reduced:")


@pytest.mark.skipif(H.device_count() > 0, reason="a GPU is present")
def test_without_a_device_the_calls_answer_nodevice(grid):
    h = np.ones((2, 8, 1), np.uint64)
    with pytest.raises(H.HareError) as ei:
        grid.hist_reduce(h, windows=[(0, 8)], levels=[1 << 31])
    assert ei.value.code == capi.HARE_E_NODEVICE
    with pytest.raises(H.HareError) as ei:
        grid.hist_reduce_device(2, 8, 1, 1, h.ctypes.data, h.ctypes.data + 4096, h.ctypes.data + 8192, windows=[(0, 8)], levels=[5])
    assert ei.value.code == capi.HARE_E_NODEVICE
    rays = np.zeros((8, 6))
    rays[:, 3] = 1.0
    for call in (lambda: grid.Receive_batch_reduced(rays, 2, 4, 0.5, windows=[(0, 4)]),
                 lambda: grid.Receive_source_reduced(8, 2, 4, 0.5, levels=[7])):
        with pytest.raises(H.HareError) as ei:
            call()
        assert ei.value.code == capi.HARE_E_NODEVICE


def test_decay_levels_and_air_weights_at_hand_computed_points():
    lv = H.decay_levels([0, -5, -10, -20, -35])
    assert lv.dtype == np.uint32
    # 10^-0.5 * 2^32 = 1358187913.3..., 10^-1 * 2^32 = 429496729.6, 10^-2 * 2^32 = 42949672.96, 10^-3.5 * 2^32 = 1358187.9...
    assert lv.tolist() == [4294967295, 1358187913, 429496729, 42949672, 1358187]
    with pytest.raises(ValueError):
        H.decay_levels([3.0])
    w = H.air_weights([0.0, math.log(2.0), 100.0], 1.0, 3)
    assert w.dtype == np.uint32 and w.shape == (3, 3)
    assert w[:, 0].tolist() == [4294967295] * 3                               # m = 0: as near 1.0 as a weight gets
    # exp(-ln 2 * (i + 0.5)) = 2^-(i + 0.5): 2^31.5 = 3037000499.97..., halved per bin
    assert abs(int(w[0, 1]) - 3037000499) <= 1 and abs(int(w[1, 1]) - 1518500249) <= 1 and abs(int(w[2, 1]) - 759250124) <= 1
    assert w[:, 2].tolist() == [0, 0, 0]                                      # exp(-50) * 2^32 < 1
    s0, s1 = H.sums_to_float(np.array([[3, 1, 5, 0]], np.uint64))
    assert s0[0] == 3 + 2.0 ** 64 and s1[0] == 5.0


def test_the_two_restatements_agree():
    rng = np.random.default_rng(5)
    for B, ch in ((1, 1), (3, 4)):
        h = rng.integers(0, 1 << 63, (2, 37, B) + ((4,) if ch == 4 else ()), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        h[0, 20:] = 0
        w = rng.integers(0, 1 << 32, (37, B), dtype=np.uint64).astype(np.uint32)
        win = [(0, 0), (0, 37), (5, 6), (3, 30), (36, 37)]
        lv = [0, 1, (1 << 32) - 1, 1 << 31] + H.decay_levels([-5, -25]).tolist()
        for weight in (None, w):
            a, b = reduce_direct(h, win, lv, weight), reduce_ref(h, win, lv, weight)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    z = reduce_ref(np.zeros((1, 4, 1), np.uint64), [(0, 4)], [0, 5])
    assert not z[0].any() and not z[1].any()                                  # T = 0 gives 0


def test_exponential_decay_crossings_and_centre_time():
    n = 600
    h = np.array([int(math.floor(2.0 ** 40 * 10.0 ** (-6.0 * i / n))) for i in range(n)], np.uint64).reshape(1, n, 1)
    _, cross = reduce_ref(h, [], H.decay_levels([-5, -25, -35]))
    # R(i) / T = (10^(-6 i / n) - 10^-6) / (1 - 10^-6) for the continuous decay: the level L dB is met at i = -(n / 6) log10(10^(L / 10) (1 - 10^-6) + 10^-6)
    for got, dB in zip(cross[0, 0], (-5, -25, -35)):
        want = -(n / 6.0) * math.log10(10.0 ** (dB / 10.0) * (1 - 1e-6) + 1e-6)
        assert abs(int(got) - want) <= 1.0, (dB, got, want)
    one = np.zeros((1, 50, 2), np.uint64)
    one[0, 17, 0], one[0, 49, 1] = 12345, (1 << 64) - 1
    sums, _ = reduce_ref(one, [(0, 50)], [])
    for b, at in ((0, 17), (1, 49)):
        s0 = int(sums[0, b, 0, 0]) + (int(sums[0, b, 0, 1]) << 64)
        s1 = int(sums[0, b, 0, 2]) + (int(sums[0, b, 0, 3]) << 64)
        assert s1 == at * s0 and s0 > 0
