"""The image-source kernels (hare_amd/csrc/image.hip) keep their working set in registers: no VGPR spilled, no scratch, and a VGPR bound
per kernel that keeps the occupancy class the build reports -- 128 for hare_image_pairs (118 VGPRs: four waves per SIMD), 64 for the
mirror (28) and the deposits (36 / 44): eight waves per SIMD -- read from the metadata the compiler
writes next to the code object, as tests/test_direct_kernel_resources.py does for the direct sound.  The deposit adds with 64-bit integer
atomics, never a compare-and-swap loop, and takes FP64 sqrt as the correctly rounded expansion, never the raw instruction; the pair search
reads its receivers from LDS and appends with one 64-bit atomic."""
import pytest

from tests.test_kernel_resources import kernels
from tests.test_receive_kernel_resources import body, built

IMAGE = ("hare_image_mirror", "hare_image_pairs", "hare_image_deposit", "hare_image_deposit_dir")
VGPRS = {"hare_image_mirror": 64, "hare_image_pairs": 128, "hare_image_deposit": 64, "hare_image_deposit_dir": 64}


@built
@pytest.mark.parametrize("name", IMAGE)
def test_image_kernels_spill_nothing_and_keep_their_occupancy_class(name):
    k = kernels()
    assert name in k
    r = k[name]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert "scratch_" not in body(name)
    assert r["vgpr_count"] <= VGPRS[name], r


@built
@pytest.mark.parametrize("name", IMAGE[2:])
def test_the_deposit_adds_with_64_bit_integer_atomics(name):
    b = body(name)
    assert "global_atomic_add_x2" in b and "cmpswap" not in b
    assert "v_sqrt_f64" not in b


@built
def test_the_pair_search_streams_its_receivers_from_lds_and_appends_with_one_atomic():
    b = body("hare_image_pairs")
    assert "ds_read" in b and b.count("global_atomic_add_x2") == 1 and "cmpswap" not in b
