"""The directional kernels (hare_amd/csrc/receive.hip; HARE_RECEIVE_DIRECTIONAL) within the bounds of the kernels they stand in for: the
three receive kernels spill no VGPR, use no scratch and at most 128 VGPRs (four waves per SIMD) although they carry four channels per
histogram word; hare_rain_step_dir spills nothing and uses no scratch; all four add with 64-bit integer atomics and take FP64 sqrt as the
correctly rounded expansion, never the raw instruction -- read from the metadata the compiler writes next to the code object
(hare_amd/csrc/build/hare_kernels.s), as tests/test_rain_kernel_resources.py does."""
import os

import pytest

from tests.test_kernel_resources import ASM, kernels

RECEIVE = ("hare_receive_reflect_dir", "hare_receive_scatter_dir", "hare_receive_scatter_rain_dir")
ALL = RECEIVE + ("hare_rain_step_dir",)


@pytest.mark.skipif(not os.path.exists(ASM), reason="the library was not built here (no hare_kernels.s)")
def test_directional_kernels_spill_nothing():
    k = kernels()
    for name in ALL:
        assert name in k, name
        r = k[name]
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
    for name in RECEIVE:
        assert k[name]["vgpr_count"] <= 128, (name, k[name])


@pytest.mark.skipif(not os.path.exists(ASM), reason="the library was not built here (no hare_kernels.s)")
def test_directional_kernels_add_with_64_bit_atomics_and_no_raw_sqrt():
    txt = open(ASM).read()
    for name in ALL:
        start = txt.index("\n" + name + ":")
        body = txt[start:txt.index(".Lfunc_end", start)]
        assert "global_atomic_add_x2" in body and "cmpswap" not in body, name
        assert "v_sqrt_f64" not in body, name
        assert "scratch_" not in body, name
