"""The 36 kernels that add histogram words (hare_amd/csrc/receive.hip, direct.hip, image.hip, image2.hip: five receive kernels, hare_rain_step
and the three deposits, each in four channel forms) after their band writer (hist_add), their stream draw (scatter_base) and their entry
points (HARE_CHANNEL_FORMS) were folded into shared pieces: each uses no more vector registers than the parent commit's build did and
exactly its LDS, and spills nothing.  The parent's figures are tests/golden/receive_pieces/parent_resources.json, read from the metadata
of that build (hare_kernels.s), not chosen here: the output of tools/kernel_resources.py on a build of the parent commit (the recipe is in
that tool's docstring)."""
import importlib.util
import json
import os

import pytest

from tests.test_kernel_resources import ASM
from tests.test_receive_kernel_resources import body, built

HERE = os.path.dirname(os.path.abspath(__file__))
PARENT = json.load(open(os.path.join(HERE, "golden", "receive_pieces", "parent_resources.json")))
PREFIXES = ["hare_receive", "hare_rain", "hare_direct_deposit", "hare_image_deposit", "hare_image2_deposit"]
FORMS = ("", "_dir", "_dir2", "_dir3")
BASES = ("hare_receive_reflect", "hare_receive_scatter", "hare_receive_scatter_rain", "hare_receive_reflect_map", "hare_receive_scatter_map",
         "hare_rain_step", "hare_direct_deposit", "hare_image_deposit", "hare_image2_deposit")


def kernels():
    """This build's figures, through the parser that wrote the parent's"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(os.path.dirname(HERE), "tools", "kernel_resources.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.resources(ASM, PREFIXES)


def test_the_record_holds_the_36_kernels():
    assert sorted(PARENT) == sorted(b + f for b in BASES for f in FORMS)


@built
def test_the_build_has_the_parents_kernels_and_no_other():
    assert sorted(kernels()) == sorted(PARENT)


@built
@pytest.mark.parametrize("name", sorted(PARENT))
def test_histogram_kernels_keep_the_parents_registers_and_lds(name):
    r, was = kernels()[name], PARENT[name]
    print(name, "vgpr", r["vgpr_count"], "parent", was["vgpr_count"], "lds", r["group_segment_fixed_size"], "parent", was["group_segment_fixed_size"])
    assert r["vgpr_count"] <= was["vgpr_count"], (r, was)
    assert r["group_segment_fixed_size"] == was["group_segment_fixed_size"], (r, was)
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    assert "scratch_" not in body(name)
