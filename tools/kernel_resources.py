"""Register and scratch figures of kernels from the metadata the compiler writes next to the code object (hare_amd/csrc/build/hare_kernels.s,
made by the library's Makefile): for every kernel whose name starts with one of the prefixes, vgpr_count, sgpr_count,
private_segment_fixed_size (scratch), vgpr_spill_count and group_segment_fixed_size (LDS).  Prints ONE JSON object, keys sorted.
tests/golden/image2/parent_receive_resources.json is this tool's output on a build of the parent commit of the second-order image sources:
  git worktree add /tmp/parent <parent commit> && make -C /tmp/parent/hare_amd/csrc all
  python tools/kernel_resources.py /tmp/parent/hare_amd/csrc/build/hare_kernels.s hare_receive hare_rain > tests/golden/image2/parent_receive_resources.json
tests/golden/deposits/parent_resources.json is its output on a build of the parent commit of the shared deposit (deposit.hip), twelve kernels:
  python tools/kernel_resources.py /tmp/parent/hare_amd/csrc/build/hare_kernels.s hare_direct hare_image > tests/golden/deposits/parent_resources.json
tests/golden/receive_pieces/parent_resources.json is its output on a build of the parent commit of the shared band writer (hist_add), the 36
kernels that add histogram words:
  python tools/kernel_resources.py /tmp/parent/hare_amd/csrc/build/hare_kernels.s hare_receive hare_rain hare_direct_deposit hare_image_deposit hare_image2_deposit > tests/golden/receive_pieces/parent_resources.json
profiles/image2/kernel_resources.json is its output for `hare_image2` on this tree's build.
usage: python tools/kernel_resources.py hare_kernels.s PREFIX [PREFIX ..]"""
import json
import re
import sys


def resources(path, prefixes):
    txt = open(path).read()
    meta = txt[txt.index("amdhsa.kernels:"):]
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        def g(key):
            return re.search(r"\." + key + r":\s+(\S+)", blk).group(1)
        name = g("name")
        if any(name.startswith(p) for p in prefixes):
            out[name] = {k: int(g(k)) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")}
    return out


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    print(json.dumps(resources(sys.argv[1], sys.argv[2:]), indent=1, sort_keys=True))
