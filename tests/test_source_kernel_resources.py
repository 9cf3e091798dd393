"""hare_emit_source (hare_amd/csrc/source.hip) keeps its working set in registers, in the manner of tests/test_receive_kernel_resources.py:
no VGPR spilled, no scratch, at most 128 VGPRs (that file's bound: four waves per SIMD) -- read from the metadata the compiler writes
next to the code object.  Its FP64 sqrt is the correctly rounded expansion, never the raw instruction; it adds nothing atomically (every
lane writes its own ray and state words)."""
import pytest

from tests.test_kernel_resources import kernels
from tests.test_receive_kernel_resources import body, built

NAME = "hare_emit_source"


@built
def test_emit_kernel_spills_nothing():
    k = kernels()
    assert NAME in k
    r = k[NAME]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert "scratch_" not in body(NAME)
    assert r["vgpr_count"] <= 128, r


@built
def test_emit_kernel_rounds_correctly_and_only_stores():
    b = body(NAME)
    assert "v_sqrt_f64" not in b and "v_rsq_f64" in b                          # the refined expansion
    assert "v_div_scale_f64" in b and "v_div_fixup_f64" in b                   # the correctly rounded division of the texel lookup
    assert "atomic" not in b and "global_store" in b
