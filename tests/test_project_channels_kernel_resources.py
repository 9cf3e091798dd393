"""hare_hist_project_channels (hare_amd/csrc/project_channels.hip) keeps its working set in registers, in the manner of
tests/test_project_kernel_resources.py: the kernel is in the code object, spills no register and uses no scratch, its LDS is static and
under 64 KiB, and its by-value arguments are the projection's -- read from the resource notes the compiler writes next to the code
object, and from nothing else.  The VGPR count and the occupancy that follows from it and from the LDS are reported (-s shows them) and
held inside the four waves per SIMD DESIGN.md 7b "Directional projection" states."""
from tests.test_kernel_resources import kernels
from tests.test_project_kernel_resources import metadata
from tests.test_receive_kernel_resources import built

NAME = "hare_hist_project_channels"
LDS_PER_CU = 160 * 1024


def occupancy(vgprs, lds):
    """waves per SIMD of a workgroup of four waves: by registers (a 512-entry file, granule 8) and by LDS (workgroups per CU = waves per SIMD)"""
    alloc = (vgprs + 7) // 8 * 8
    return min(8, 512 // alloc), min(8, LDS_PER_CU // lds)


@built
def test_project_channels_kernel_is_there_and_spills_nothing():
    k = kernels()
    assert NAME in k
    r = k[NAME]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    m = metadata(NAME)
    assert m["sgpr_spill_count"] == 0 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    by_regs, by_lds = occupancy(r["vgpr_count"], m["group_segment_fixed_size"])
    print(f"{NAME}: {r['vgpr_count']} VGPRs, {m['group_segment_fixed_size']} bytes of LDS: {by_regs} waves per SIMD by registers, {by_lds} by LDS")
    assert r["vgpr_count"] <= 128 and by_regs >= 4 and by_lds >= 4, (r, m)          # four waves per SIMD either way


@built
def test_project_channels_kernel_lds_is_static_and_its_arguments_are_the_projections():
    m = metadata(NAME)
    # 4 quantities x 4 partials x 128 pairs x 16 bytes, 128 x 16 for 2^31 T and 4 x 8 x 8 for the coefficient sums
    assert m["group_segment_fixed_size"] == 4 * 4 * 128 * 16 + 128 * 16 + 4 * 8 * 8 < 64 * 1024, m
    assert m["kernarg_segment_size"] == metadata("hare_hist_project")["kernarg_segment_size"] == 48, m          # four pointers and four int32 by value
