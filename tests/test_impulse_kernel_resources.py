"""hare_hist_impulses (hare_amd/csrc/impulses.hip) keeps a sample's sums of all sixteen channels in registers across the bands, in the
manner of tests/test_convolve_kernel_resources.py: the kernel is in the code object, spills no VGPR and uses no scratch -- read from the
metadata the compiler writes next to the code object.  Its arithmetic is the definition's: FP64 multiplies and FP64 adds, and no fused
multiply-add anywhere in its body -- the contraction include/hare_hip.h ("Impulses") forbids.  Its dynamic LDS is the plan's figure and
fits a CU.  Resources only."""
import re

from tests.test_kernel_resources import kernels
from tests.test_receive_kernel_resources import body, built

NAME = "hare_hist_impulses"


@built
def test_impulse_kernel_is_there_and_spills_nothing():
    k = kernels()
    assert NAME in k
    r = k[NAME]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert "scratch_" not in body(NAME)
    assert r["vgpr_count"] <= 128, r          # a workgroup of 256 threads: at least two of them on a CU as far as registers go


@built
def test_impulse_kernel_multiplies_then_adds():
    b = body(NAME)
    ops = re.findall(r"^\s+(v_[a-z0-9_]+)", b, flags=re.M)
    # the walk of each channel count unrolled: 1 + 4 + 9 + 16 pairs
    assert ops.count("v_mul_f64") >= 30 and ops.count("v_add_f64") >= 30, (ops.count("v_mul_f64"), ops.count("v_add_f64"))
    assert "v_fma_f64" not in b and not [o for o in ops if "fma" in o and "f64" in o], "a fused multiply-add"


def test_impulse_kernel_lds_is_within_the_plans_figure():
    """impulses_plan (hist.cpp): the taps and one chunk's list; the largest shape, 8 bands of 1024 taps at 16 channels, within a CU's 160 KiB;
    the measured shape (8 x 511 taps, 16 channels) leaves room for two workgroups"""
    from tests.impulse_cases import plan
    assert plan(1, 8, 16, 1024, 1)[2] == 103440 <= 160 * 1024
    assert 2 * plan(1, 8, 16, 511, 1)[2] <= 160 * 1024
