"""The projection of a histogram (include/hare_hip.h, "receivers", "Projection") without a GPU: the two exports are bound and declared;
every refusal of the header is HARE_E_INVALID, in the header's order, with a message that names the call; behind the checks a GPU-less
host answers HARE_E_NODEVICE; and the restatement's own sanity (tests/project_ref.py): its two forms agree, and ones and c = i give the
S0 and S1 of the reduction's restatement over the full window."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests.project_ref import project_direct, project_ints, project_ref, to_int
from tests.reduce_ref import reduce_ref

NEW = ("hare_hist_project_device", "hare_hist_project")


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
    assert "Projection (hare_hist_project_device, hare_hist_project)" in hdr


ARENA = np.zeros(1 << 16, np.uint64)          # any non-null addresses: nothing is dereferenced before the checks pass
A0 = ARENA.ctypes.data


def call(grid, dev, K=2, n_bins=8, B=1, channels=1, hist=A0, weight=None, J=3, coef=A0 + 65536, proj=A0 + 131072):
    """Either call on raw addresses: (rc, message)."""
    if dev:
        rc = capi.lib.hare_hist_project_device(grid._h, K, n_bins, B, channels, hist, weight, J, coef, proj, None)
    else:
        rc = capi.lib.hare_hist_project(grid._h, K, n_bins, B, channels, hist, weight, J, coef, proj)
    return rc, capi.last_error()


SHAPE = [dict(K=0), dict(K=65537), dict(n_bins=0), dict(n_bins=-1), dict(B=0), dict(B=9), dict(channels=0), dict(channels=2), dict(channels=3),
         dict(channels=5), dict(K=65536, n_bins=1025, B=2), dict(K=4096, n_bins=4097, B=2, channels=4)]
VECTORS = [dict(J=0), dict(J=-1), dict(J=33)]
NULLS = [dict(hist=None), dict(coef=None), dict(proj=None)]
# proj is 2 x 1 x 3 x 2 x 8 = 96 bytes, hist 128, coef 96, weight 32
OVERLAPS = [dict(proj=A0), dict(proj=A0 + 120), dict(hist=A0 + 131072 + 88), dict(proj=A0 + 65536 + 92), dict(weight=A0 + 131072 + 95),
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
    assert msg.startswith("hare_hist_project_device:" if dev else "hare_hist_project:"), msg


def test_a_null_scene_is_refused():
    assert capi.lib.hare_hist_project(None, 2, 8, 1, 1, A0, None, 3, A0 + 65536, A0 + 131072) == capi.HARE_E_INVALID
    assert capi.lib.hare_hist_project_device(None, 2, 8, 1, 1, A0, None, 3, A0 + 65536, A0 + 131072, None) == capi.HARE_E_INVALID


@pytest.mark.parametrize("dev", (False, True), ids=("host", "device"))
def test_the_refusals_come_in_the_headers_order(grid, dev):
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
    # adjacent buffers do not overlap, and a weight beside the output is fine: these get past every check
    if H.device_count() == 0:
        for kw in (dict(proj=A0 + 128), dict(proj=A0 + 65536 + 96), dict(weight=A0 + 131072 + 96), dict(weight=A0 + 131072 - 32)):
            rc, msg = call(grid, dev, **kw)
            assert rc == capi.HARE_E_NODEVICE, (kw, rc, msg)


@pytest.mark.skipif(H.device_count() > 0, reason="a GPU is present")
def test_without_a_device_the_calls_answer_nodevice(grid):
    h = np.ones((2, 8, 1), np.uint64)
    c = np.ones((3, 8), np.int32)
    with pytest.raises(H.HareError) as ei:
        grid.hist_project(h, c)
    assert ei.value.code == capi.HARE_E_NODEVICE
    with pytest.raises(H.HareError) as ei:
        grid.hist_project_device(2, 8, 1, 1, A0, 3, A0 + 65536, A0 + 131072)
    assert ei.value.code == capi.HARE_E_NODEVICE
    for J in (1, 32):                                                        # the ends of the range are inside it
        assert call(grid, True, J=J)[0] == capi.HARE_E_NODEVICE


def test_the_python_wrapper_checks_shapes_and_never_wraps_a_coefficient(grid):
    h = np.ones((2, 8, 1), np.uint64)
    for bad in (np.ones((3, 7), np.int32), np.ones(8, np.int32), np.ones((0, 8), np.int32), np.full((1, 8), 1 << 31, np.int64),
                np.full((1, 8), -(1 << 31) - 1, np.int64), np.ones((1, 8), np.float64)):
        with pytest.raises(ValueError):
            grid.hist_project(h, bad)
    with pytest.raises(ValueError):
        grid.hist_project(np.ones((2, 8), np.uint64), np.ones((1, 8), np.int32))
    p = np.array([[5, 0], [(1 << 64) - 1, (1 << 64) - 1], [0, 1 << 63], [1, 1]], np.uint64)
    assert H.proj_to_int(p).tolist() == [5, -1, -(1 << 127), (1 << 64) + 1]


def test_the_two_restatements_agree():
    rng = np.random.default_rng(11)
    for B, ch in ((1, 1), (3, 4), (2, 9)):
        h = rng.integers(0, 1 << 64, (2, 37, B) + ((ch,) if ch > 1 else ()), dtype=np.uint64)
        h[0, 20:] = np.uint64((1 << 64) - 1)
        w = rng.integers(0, 1 << 32, (37, B), dtype=np.uint64).astype(np.uint32)
        c = rng.integers(-(1 << 31), 1 << 31, (6, 37), dtype=np.int64).astype(np.int32)
        c[0], c[1], c[2] = -(1 << 31), (1 << 31) - 1, -1
        for weight in (None, w):
            a, b = project_direct(h, c, weight), project_ref(h, c, weight)
            assert a.dtype == b.dtype == np.uint64 and a.shape == b.shape == (2, B, 6, 2) and np.array_equal(a, b)
            assert (to_int(b) == project_ints(h, c, weight)).all()
    z = project_ref(np.zeros((1, 4, 1), np.uint64), np.full((2, 4), -5, np.int32))
    assert not z.any()
    one = project_ref(np.array([[[3]], [[4]]], np.uint64), np.array([[-2]], np.int32))          # -6 and -8 in two's complement
    assert one.reshape(2, 2).tolist() == [[(1 << 64) - 6, (1 << 64) - 1], [(1 << 64) - 8, (1 << 64) - 1]]


def test_ones_and_the_bin_index_give_the_reductions_sums():
    rng = np.random.default_rng(12)
    n = 300
    h = rng.integers(0, 1 << 64, (3, n, 5), dtype=np.uint64)
    w = rng.integers(0, 1 << 32, (n, 5), dtype=np.uint64).astype(np.uint32)
    c = np.stack([np.ones(n, np.int32), np.arange(n, dtype=np.int32)])
    for weight in (None, w):
        sums, _ = reduce_ref(h, [(0, n)], [], weight)
        p = project_ref(h, c, weight)
        assert np.array_equal(p[:, :, 0], sums[:, :, 0, 0:2]) and np.array_equal(p[:, :, 1], sums[:, :, 0, 2:4])
