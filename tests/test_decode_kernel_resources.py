"""hare_decode (hare_amd/csrc/decode.hip) keeps its accumulators and its window of the input channel in registers across the channel loop,
in the manner of tests/test_convolve_kernel_resources.py: the kernel is in the code object, spills no VGPR, uses no scratch and fits four
waves per SIMD -- read from the metadata the compiler writes next to the code object.  Its arithmetic is the definition's: FP64 multiplies
and FP64 adds, and no fused multiply-add anywhere in its body -- the contraction include/hare_hip.h ("Decoding") forbids.  Resources only."""
import re

from tests.test_kernel_resources import kernels
from tests.test_receive_kernel_resources import body, built

NAME = "hare_decode"


@built
def test_decode_kernel_is_there_and_spills_nothing():
    k = kernels()
    assert NAME in k
    r = k[NAME]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert "scratch_" not in body(NAME)
    assert r["vgpr_count"] <= 128, r          # four waves per SIMD: four workgroups of 256 threads on a CU


@built
def test_decode_kernel_multiplies_then_adds():
    b = body(NAME)
    ops = re.findall(r"^\s+(v_[a-z0-9_]+)", b, flags=re.M)
    assert ops.count("v_mul_f64") >= 256 and ops.count("v_add_f64") >= 256, (ops.count("v_mul_f64"), ops.count("v_add_f64"))
    assert "v_fma_f64" not in b and not [o for o in ops if "fma" in o], "a fused multiply-add"


@built
def test_decode_kernel_lds_leaves_four_workgroups_to_a_cu():
    """decode_plan's dynamic LDS (hare_device.h: kDecodeLdsDoubles, the convolution's) four times over fits the 160 KiB of a CU"""
    from tests.decode_cases import LDS_BYTES
    assert 4 * LDS_BYTES <= 160 * 1024
