"""hare_hist_render (hare_amd/csrc/render.hip) keeps its accumulators and its sign window in registers, in the manner of
tests/test_hist_reduce_kernel_resources.py: the kernel is in the code object, spills no VGPR and uses no scratch -- read from the metadata
the compiler writes next to the code object.  Resources only."""
from tests.test_kernel_resources import kernels
from tests.test_receive_kernel_resources import built

NAME = "hare_hist_render"


@built
def test_render_kernel_is_there_and_spills_nothing():
    k = kernels()
    assert NAME in k
    r = k[NAME]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 128, r          # four waves per SIMD: two workgroups of 512 threads on a CU
