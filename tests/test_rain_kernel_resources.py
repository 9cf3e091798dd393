"""Diffuse rain's kernels (hare_amd/csrc/receive.hip) within the bounds of the receive kernels: hare_rain_step and hare_receive_scatter_rain
spill no VGPR, use no scratch and at most 128 VGPRs (four waves per SIMD), add the histogram with 64-bit integer atomics and take FP64 sqrt
as the correctly rounded expansion, never the raw instruction -- read from the metadata the compiler writes next to the code object
(hare_amd/csrc/build/hare_kernels.s), as tests/test_scatter_kernel_resources.py does."""
import os

import pytest

from tests.test_kernel_resources import ASM, kernels

RAIN = ("hare_rain_step", "hare_receive_scatter_rain")


@pytest.mark.skipif(not os.path.exists(ASM), reason="the library was not built here (no hare_kernels.s)")
def test_rain_kernels_spill_nothing():
    k = kernels()
    for name in RAIN:
        assert name in k, name
        r = k[name]
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["vgpr_count"] <= 128, (name, r)


@pytest.mark.skipif(not os.path.exists(ASM), reason="the library was not built here (no hare_kernels.s)")
def test_rain_kernels_add_with_64_bit_atomics_and_no_raw_sqrt():
    txt = open(ASM).read()
    for name in RAIN:
        start = txt.index(name + ":")
        body = txt[start:txt.index(".Lfunc_end", start)]
        assert "global_atomic_add_x2" in body and "cmpswap" not in body, name
        assert "v_sqrt_f64" not in body, name
