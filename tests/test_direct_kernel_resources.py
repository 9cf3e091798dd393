"""The direct sound's kernels (hare_amd/csrc/direct.hip) keep their working set in registers: no VGPR spilled, no scratch, at most 128
VGPRs -- read from the metadata the compiler writes next to the code object, as tests/test_receive_kernel_resources.py does for the receive
kernels.  The deposit adds with 64-bit integer atomics, never a compare-and-swap loop, and takes FP64 sqrt as the correctly rounded
expansion, never the raw instruction."""
import pytest

from tests.test_kernel_resources import kernels
from tests.test_receive_kernel_resources import body, built

DIRECT = ("hare_direct_emit", "hare_direct_deposit", "hare_direct_deposit_dir")


@built
@pytest.mark.parametrize("name", DIRECT)
def test_direct_kernels_spill_nothing_and_stay_within_128_vgprs(name):
    k = kernels()
    assert name in k
    r = k[name]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert "scratch_" not in body(name)
    assert r["vgpr_count"] <= 128, r


@built
@pytest.mark.parametrize("name", DIRECT[1:])
def test_the_deposit_adds_with_64_bit_integer_atomics(name):
    b = body(name)
    assert "global_atomic_add_x2" in b and "cmpswap" not in b
    assert "v_sqrt_f64" not in b
