"""The receiver-map kernels (hare_amd/csrc/receive.hip, the _map forms) keep their working set in registers: no VGPR spilled, no scratch,
at most 128 VGPRs (four waves per SIMD) -- read from the metadata the compiler writes next to the code object, as
tests/test_receive_kernel_resources.py does for their siblings.  They add with 64-bit integer atomics, never a compare-and-swap loop,
and take FP64 sqrt as the correctly rounded expansion, never the raw instruction."""
import pytest

from tests.test_kernel_resources import kernels
from tests.test_receive_kernel_resources import body, built

MAP = ("hare_receive_reflect_map", "hare_receive_scatter_map", "hare_receive_reflect_map_dir", "hare_receive_scatter_map_dir")


@built
@pytest.mark.parametrize("name", MAP)
def test_map_kernels_spill_nothing_and_stay_within_128_vgprs(name):
    k = kernels()
    assert name in k
    r = k[name]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert "scratch_" not in body(name)
    assert r["vgpr_count"] <= 128, r


@built
@pytest.mark.parametrize("name", MAP)
def test_map_kernels_add_with_64_bit_integer_atomics(name):
    b = body(name)
    assert "global_atomic_add_x2" in b and "cmpswap" not in b
    assert "v_sqrt_f64" not in b
