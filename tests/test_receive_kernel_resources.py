"""hare_receive_reflect (hare_amd/csrc/receive.hip) keeps its working set in registers: no VGPR spilled, no scratch, and at most 128
VGPRs (four waves per SIMD) -- read from the metadata the compiler writes next to the
code object (hare_amd/csrc/build/hare_kernels.s, made by the library's Makefile), as tests/test_kernel_resources.py does for the shoot
kernels.  Its receivers live in LDS (8 KiB for 256 spheres); the histogram is added with 64-bit integer atomics."""
import os

import pytest

from tests.test_kernel_resources import ASM, kernels


@pytest.mark.skipif(not os.path.exists(ASM), reason="the library was not built here (no hare_kernels.s)")
def test_receive_kernel_spills_nothing():
    k = kernels()
    assert "hare_receive_reflect" in k
    r = k["hare_receive_reflect"]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 128, r


@pytest.mark.skipif(not os.path.exists(ASM), reason="the library was not built here (no hare_kernels.s)")
def test_receive_kernel_adds_the_histogram_with_64_bit_integer_atomics():
    txt = open(ASM).read()
    start = txt.index("hare_receive_reflect:")
    body = txt[start:txt.index(".Lfunc_end", start)]
    assert "global_atomic_add_x2" in body and "cmpswap" not in body
    assert "ds_read" in body                                                 # the receivers are read from LDS
