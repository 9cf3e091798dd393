"""The receive loop's kernels (hare_amd/csrc/receive.hip) keep their working set in registers: no VGPR spilled, no scratch, and at most
128 VGPRs (four waves per SIMD; hare_rain_step_dir, which holds four channels per band next to its shadow walk, is not held to that) --
read from the metadata the compiler writes next to the code object (hare_amd/csrc/build/hare_kernels.s, made by the library's Makefile),
as tests/test_kernel_resources.py does for the shoot kernels.  The histogram is added with 64-bit integer atomics, never a compare-and-swap
loop; the receive kernels read their receivers from LDS (8 KiB for 256 spheres); FP64 sqrt is the correctly rounded expansion, never the
raw instruction (hare_receive_reflect takes no sqrt)."""
import os

import pytest

from tests.test_kernel_resources import ASM, kernels

RECEIVE = ("hare_receive_reflect", "hare_receive_scatter", "hare_receive_scatter_rain",
           "hare_receive_reflect_dir", "hare_receive_scatter_dir", "hare_receive_scatter_rain_dir")
RAIN = ("hare_rain_step", "hare_rain_step_dir")
built = pytest.mark.skipif(not os.path.exists(ASM), reason="the library was not built here (no hare_kernels.s)")


def body(name):
    txt = open(ASM).read()
    start = txt.index("\n" + name + ":")
    return txt[start:txt.index(".Lfunc_end", start)]


@built
@pytest.mark.parametrize("name", RECEIVE + RAIN)
def test_receive_kernels_spill_nothing(name):
    k = kernels()
    assert name in k
    r = k[name]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert "scratch_" not in body(name)
    if name != "hare_rain_step_dir":
        assert r["vgpr_count"] <= 128, r


@built
@pytest.mark.parametrize("name", RECEIVE + RAIN)
def test_receive_kernels_add_the_histogram_with_64_bit_integer_atomics(name):
    b = body(name)
    assert "global_atomic_add_x2" in b and "cmpswap" not in b
    assert "v_sqrt_f64" not in b
    if name in RECEIVE:
        assert "ds_read" in b                                                # the receivers are read from LDS
