"""The second-order image-source kernels (hare_amd/csrc/image2.hip) keep their working set in registers -- no VGPR spilled, no scratch --
and the receive kernels, which gained the byte per ray of HARE_RECEIVE_IMAGE2, use no more vector registers and no more scratch than the
parent commit's build did: its figures are tests/golden/image2/parent_receive_resources.json, read from the metadata of that build
(hare_kernels.s), not chosen here: it is the output of tools/kernel_resources.py on a build of the parent commit (the recipe is in that
tool's docstring; regenerate it whenever the parent's receive kernels change).  Vector registers and scratch are what bound a wave's
occupancy on gfx950; that parser reads no scalar counts, and the file records the parent's for the reader."""
import json
import os

import pytest

from tests.test_kernel_resources import kernels
from tests.test_receive_kernel_resources import body, built

IMAGE2 = ("hare_image2_mirror", "hare_image2_cands", "hare_image2_paths", "hare_image2_deposit", "hare_image2_deposit_dir")
PARENT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image2", "parent_receive_resources.json")))


@built
@pytest.mark.parametrize("name", IMAGE2)
def test_image2_kernels_spill_nothing(name):
    k = kernels()
    assert name in k
    r = k[name]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert "scratch_" not in body(name)
    assert r["vgpr_count"] <= 256, r


@built
def test_the_two_searches_stream_from_lds_and_append_with_one_atomic():
    for name in ("hare_image2_cands", "hare_image2_paths"):
        b = body(name)
        assert "ds_read" in b and b.count("global_atomic_add_x2") == 1 and "cmpswap" not in b, name


@built
@pytest.mark.parametrize("name", sorted(PARENT))
def test_receive_kernels_use_no_more_registers_than_the_parent(name):
    r, was = kernels()[name], PARENT[name]
    print(name, "vgpr", r["vgpr_count"], "parent", was["vgpr_count"])
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0
    assert r["vgpr_count"] <= was["vgpr_count"], (r, was)
