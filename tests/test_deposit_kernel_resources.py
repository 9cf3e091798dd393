"""The twelve kernels of the deterministic source paths (hare_amd/csrc/direct.hip, image.hip, image2.hip) after their deposits, appends and
argument structs were folded into shared pieces (deposit.hip, DepositArgs): each uses no more vector registers than the parent commit's
build did and exactly its LDS, and spills nothing.  The parent's figures are tests/golden/deposits/parent_resources.json, read from the
metadata of that build (hare_kernels.s), not chosen here: the output of tools/kernel_resources.py on a build of the parent commit (the
recipe is in that tool's docstring)."""
import importlib.util
import json
import os

import pytest

from tests.test_kernel_resources import ASM
from tests.test_receive_kernel_resources import body, built

HERE = os.path.dirname(os.path.abspath(__file__))
PARENT = json.load(open(os.path.join(HERE, "golden", "deposits", "parent_resources.json")))


def kernels():
    """This build's figures, through the parser that wrote the parent's"""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(os.path.dirname(HERE), "tools", "kernel_resources.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.resources(ASM, ["hare_direct", "hare_image"])


def test_the_record_holds_the_twelve_kernels():
    assert len(PARENT) == 12 and all(n.startswith(("hare_direct_", "hare_image_", "hare_image2_")) for n in PARENT)


@built
@pytest.mark.parametrize("name", sorted(PARENT))
def test_deposit_kernels_keep_the_parents_registers_and_lds(name):
    r, was = kernels()[name], PARENT[name]
    print(name, "vgpr", r["vgpr_count"], "parent", was["vgpr_count"], "lds", r["group_segment_fixed_size"], "parent", was["group_segment_fixed_size"])
    assert r["vgpr_count"] <= was["vgpr_count"], (r, was)
    assert r["group_segment_fixed_size"] == was["group_segment_fixed_size"], (r, was)
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    assert "scratch_" not in body(name)
