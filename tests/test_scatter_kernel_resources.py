"""hare_receive_scatter (hare_amd/csrc/receive.hip) within the bounds of hare_receive_reflect: no VGPR spilled, no scratch, at most 128
VGPRs (four waves per SIMD), the histogram added with 64-bit integer atomics and the receivers read from LDS -- read from the metadata the
compiler writes next to the code object (hare_amd/csrc/build/hare_kernels.s), as tests/test_receive_kernel_resources.py does."""
import os

import pytest

from tests.test_kernel_resources import ASM, kernels


@pytest.mark.skipif(not os.path.exists(ASM), reason="the library was not built here (no hare_kernels.s)")
def test_scatter_kernel_spills_nothing():
    k = kernels()
    assert "hare_receive_scatter" in k
    r = k["hare_receive_scatter"]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 128, r


@pytest.mark.skipif(not os.path.exists(ASM), reason="the library was not built here (no hare_kernels.s)")
def test_scatter_kernel_adds_the_histogram_with_64_bit_integer_atomics():
    txt = open(ASM).read()
    start = txt.index("hare_receive_scatter:")
    body = txt[start:txt.index(".Lfunc_end", start)]
    assert "global_atomic_add_x2" in body and "cmpswap" not in body
    assert "ds_read" in body
    assert "v_sqrt_f64" not in body                                          # FP64 sqrt: the correctly rounded expansion, not the raw instruction
