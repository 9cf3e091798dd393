"""The kernels of the higher-order receivers (the _dir2 and _dir3 forms in hare_amd/csrc/receive.hip, direct.hip, image.hip and
image2.hip) keep their working set in registers: no VGPR spilled, no scratch -- read from the metadata the compiler writes next to the
code object, as tests/test_receive_kernel_resources.py reads it.  The 128 VGPRs of the first-order kernels hold for the map kernels, the
rain and the deposits.  The linear receive kernels hold a ray's polynomials (10 or 24 VGPRs) and a band's words through the receiver loop
and do not meet it: their counts are pinned here as bounds (DESIGN.md 7b says what the occupancy becomes)."""
import os

import pytest

from tests.test_kernel_resources import ASM, kernels
from tests.test_receive_kernel_resources import body

FORMS = ("hare_receive_reflect", "hare_receive_scatter", "hare_receive_scatter_rain", "hare_receive_reflect_map", "hare_receive_scatter_map",
         "hare_rain_step", "hare_direct_deposit", "hare_image_deposit", "hare_image2_deposit")
NEW = tuple(f + s for f in FORMS for s in ("_dir2", "_dir3"))
LINEAR = {"_dir2": 168, "_dir3": 216}        # VGPRs of the three linear receive kernels, as built
built = pytest.mark.skipif(not os.path.exists(ASM), reason="the library was not built here (no hare_kernels.s)")


def bound(name):
    linear = name.startswith(("hare_receive_reflect_dir", "hare_receive_scatter_dir", "hare_receive_scatter_rain_dir"))
    return LINEAR[name[-5:]] if linear else 128


@built
@pytest.mark.parametrize("name", NEW)
def test_the_higher_order_kernels_spill_nothing_and_keep_their_registers(name):
    k = kernels()
    assert name in k
    r = k[name]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert "scratch_" not in body(name)
    assert r["vgpr_count"] <= bound(name), r


@built
@pytest.mark.parametrize("name", NEW)
def test_the_higher_order_kernels_add_with_64_bit_integer_atomics(name):
    b = body(name)
    assert "global_atomic_add_x2" in b and "cmpswap" not in b
    assert "v_sqrt_f64" not in b
