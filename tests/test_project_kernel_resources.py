"""hare_hist_project (hare_amd/csrc/project.hip) keeps its working set in registers, in the manner of
tests/test_hist_reduce_kernel_resources.py: the kernel is in the code object, spills no register and uses no scratch, stays within the 128
VGPRs of four waves per SIMD, and has the static LDS and the by-value arguments DESIGN.md 7b "Projection" states -- read from the metadata
the compiler writes next to the code object.  Resources only."""
import re

from tests.test_kernel_resources import ASM, kernels
from tests.test_receive_kernel_resources import body, built

NAME = "hare_hist_project"


def metadata(name):
    txt = open(ASM).read()
    meta = txt[txt.index("amdhsa.kernels:"):]
    blk = next(b for b in re.split(r"\n  - \.agpr_count:", meta)[1:] if re.search(r"\.name:\s+" + name + r"\s", b))
    return {k: int(re.search(r"\." + k + r":\s+(\S+)", blk).group(1))
            for k in ("group_segment_fixed_size", "kernarg_segment_size", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")}


@built
def test_project_kernel_is_there_and_spills_nothing():
    k = kernels()
    assert NAME in k
    r = k[NAME]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] == 102, r          # the figure DESIGN.md states ...
    assert r["vgpr_count"] <= 128, r          # ... inside four waves per SIMD
    m = metadata(NAME)
    assert m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    assert "scratch_" not in body(NAME)


@built
def test_project_kernel_lds_and_arguments_are_what_the_design_states():
    m = metadata(NAME)
    assert m["group_segment_fixed_size"] == 4736, m          # (1 + 8) quantities x 4 waves x 8 bands x 16 bytes, and 8 x 16 for 2^31 T
    assert m["kernarg_segment_size"] == 48, m                # four pointers and four int32 by value: nothing to upload
    b = body(NAME)
    assert "global_atomic" not in b and "v_mad_u64_u32" in b
    assert not re.search(r"\bv_\w*_f(16|32|64)\b", b)        # no floating point in the kernel
