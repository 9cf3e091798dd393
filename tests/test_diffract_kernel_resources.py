"""The edge-diffraction kernels (hare_amd/csrc/diffract.hip) keep their working set in registers: no VGPR spilled, no scratch, and at most
128 VGPRs for the pair search (four waves per SIMD or more) and 64 for the emission and the deposits -- read from the metadata the compiler
writes next to the code object, as tests/test_image_kernel_resources.py does for the image sources.  The deposit adds with 64-bit integer
atomics, never a compare-and-swap loop, and FP64 sqrt is the correctly rounded expansion, never the raw instruction; the pair search reads
its receivers from LDS and appends with one 64-bit atomic."""
import pytest

from tests.test_kernel_resources import kernels
from tests.test_receive_kernel_resources import body, built

DEPOSITS = ("hare_diffract_deposit", "hare_diffract_deposit_dir", "hare_diffract_deposit_dir2", "hare_diffract_deposit_dir3")
VGPRS = dict({"hare_diffract_emit": 64, "hare_diffract_pairs": 128}, **{name: 64 for name in DEPOSITS})


@built
@pytest.mark.parametrize("name", sorted(VGPRS))
def test_diffract_kernels_spill_nothing_and_use_no_scratch(name):
    k = kernels()
    assert name in k
    r = k[name]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert "scratch_" not in body(name)
    assert r["vgpr_count"] <= VGPRS[name], r


@built
@pytest.mark.parametrize("name", DEPOSITS)
def test_the_deposit_adds_with_64_bit_integer_atomics(name):
    b = body(name)
    assert "global_atomic_add_x2" in b and "cmpswap" not in b
    assert "v_sqrt_f64" not in b


@built
def test_the_pair_search_streams_its_receivers_from_lds_and_appends_with_one_atomic():
    b = body("hare_diffract_pairs")
    assert "ds_read" in b and b.count("global_atomic_add_x2") == 1 and "cmpswap" not in b
    assert "v_sqrt_f64" not in b
