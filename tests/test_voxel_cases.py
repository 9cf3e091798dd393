"""The cases of tests/voxel_cases.py checked without a GPU: the list IS a covering array of strength 2 (every pair of levels of every two
factors, less the declared table, whose entries cannot be built), it reaches every cell of the voxel kernel table, the references have
something to decide -- counted from the oracle alone -- and they are the ones pinned in tests/golden/voxel_matrix_reference_digests.json, so
that a change of the oracle or of a ray generator is seen as that and not as a kernel's failure on the device."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

from tests.helpers import FIELDS
from tests.voxel_cases import (BOUNCES, CASES, FACTORS, FAMILIES, IMPOSSIBLE, MAX_CASES, MAX_RAYS, NAMES, ROOT, WAVE, WINDOW, Case, all_pairs,
                               grid_args, pairs_of, rays, reference, scene)

DIGESTS = os.path.join(ROOT, "tests", "golden", "voxel_matrix_reference_digests.json")


def digest(case):
    h = hashlib.sha256()
    ev = reference(case)["events"]
    for f in FIELDS:
        h.update(np.ascontiguousarray(ev[f]).tobytes())
    return h.hexdigest()


def by_kind(*kinds):
    seen, out = set(), []
    for c in CASES:
        if c.kind in kinds and c.key not in seen:
            seen.add(c.key)
            out.append(c)
    return out


def test_the_list_is_a_covering_array_of_strength_two():
    assert len(CASES) <= MAX_CASES and len({c.id for c in CASES}) == len(CASES)
    assert all(c.n <= MAX_RAYS and len(rays(c)) == c.n for c in CASES)
    seen = set()
    for c in CASES:
        seen |= pairs_of(c.levels)
    want = all_pairs()
    assert seen == want, (sorted(map(sorted, want - seen))[:5], sorted(map(sorted, seen - want))[:5])
    full = sum(len(FACTORS[a]) * len(FACTORS[b]) for i, a in enumerate(NAMES) for b in NAMES[i + 1:])
    assert len(want) == full - len(IMPOSSIBLE)


def test_a_declared_pair_cannot_be_built():
    first = {k: FACTORS[k][0] for k in NAMES}
    Case(0, **first)
    for pair, why in IMPOSSIBLE.items():
        assert why
        with pytest.raises(ValueError):
            Case(0, **dict(first, **dict(pair)))


def test_the_levels_sit_where_the_code_has_its_edges():
    """The order pass's window and the bitmap's three resolutions as the sources state them (scene.h: occ_layout, restated), the smallest
    ticket the launcher passes on unchanged, and the bounds of the adaptive grid."""
    assert FACTORS["n"] == (1, WAVE - 1, WAVE, WAVE + 1, WINDOW - 1, WINDOW + 1, 2 * WINDOW + 1) and WINDOW == 4096

    def occ_shift(ct):
        shift = 0
        while True:
            cd = (ct + (1 << shift) - 1) >> shift
            words = (cd ** 3 + 31) // 32
            if ((words + 3) // 4) * 16 <= 64 * 1024:
                return shift
            shift += 1

    scene_h = open(os.path.join(ROOT, "hare_amd", "csrc", "scene.h")).read()
    assert re.search(r"if \(\(long long\)\(\(words \+ 3\) / 4\) \* 16 <= 64 \* 1024\) return;", scene_h)
    assert [occ_shift(d) for d in (1, 8, 33, 80, 81, 160, 161)] == [0, 0, 0, 0, 1, 1, 2]
    assert occ_shift(grid_args("A7")[0]) == 0
    launch = open(os.path.join(ROOT, "hare_amd", "csrc", "launch.cpp")).read()
    assert "std::max(8, std::min(4096, o.ticket_rays))" in launch and FACTORS["ticket_rays"][1] == 8


def test_every_cell_of_the_kernel_table_has_a_case():
    """family x {fine, coarse bitmap} x {triangles, quadrilaterals} as launch.cpp's rule serves the cases; the table read from the source"""
    src = open(os.path.join(ROOT, "hare_amd", "csrc", "device_scene.cpp")).read()
    table = re.search(r"kVoxelKernelNames\[DeviceModule::kFamilies\]\[2\]\[2\] = \{(.*?)\n\};", src, re.S).group(1)
    names = re.findall(r'"(hare_voxel_\w+)"', table)
    assert len(names) == 4 * len(FAMILIES)
    cells = {c.cell for c in CASES}
    assert cells == {(f, co, q) for f in FAMILIES for co in (0, 1) for q in (0, 1)}


def test_every_scene_has_hits_and_misses():
    for name in FACTORS["scene"]:
        ev = np.concatenate([reference(c)["events"].reshape(-1) for c in CASES if c.scene == name])
        assert (ev["hit"] != 0).any() and (ev["hit"] == 0).any(), name
        tops, top, _ = scene(next(c for c in CASES if c.scene == name))
        assert (name == "tie") == bool((tops[top][1] == 3).all())


def test_the_tie_scene_has_ties():
    """the criterion of tests/test_gpu_ties.py::test_tie_scene_really_has_ties: a hit at a t that is an exact power of two"""
    plain = [reference(c)["plain"] for c in CASES if c.scene == "tie" and c.rays == "tie" and c.n > 1 and not c.adjust]
    assert plain
    ev = np.concatenate(plain)
    hit = ev["hit"] != 0
    exact = hit & np.isin(ev["t"], 2.0 ** np.arange(-4.0, 5.0))
    assert hit.sum() >= 100 and exact.sum() >= 0.10 * hit.sum(), (int(exact.sum()), int(hit.sum()))


def test_an_exclusion_changes_the_answer():
    cases = by_kind("excl")
    assert cases
    for c in cases:
        ref = reference(c)
        same = (ref["plain"]["hit"] != 0) & (ref["e1"] == ref["plain"]["poly_id"])
        assert same.sum() >= 0.25 * c.n, (c.id, int(same.sum()))
        assert (ref["e2"] < 0).any() or c.n == 1, c.id
    for c in by_kind("retired"):
        ref = reference(c)
        dead = ref["e1"] == -2
        assert dead.sum() == (c.n + 2) // 3 and ref["rays"] == c.n - dead.sum()
        assert not ref["events"]["hit"][dead].any() and (ref["events"]["poly_id"][dead] == -1).all()


def test_every_class_of_t_max_is_there():
    cases = by_kind("tmax")
    assert cases
    for c in cases:
        ref = reference(c)
        t, tm, hit = ref["plain"]["t"], ref["tmax"], ref["plain"]["hit"] != 0
        classes = {"t_max == t": hit & (tm == t), "one ulp beyond t": hit & (tm == np.nextafter(t, np.inf)), "NaN": np.isnan(tm),
                   "inf": np.isinf(tm), "-1 and 0": (tm == -1.0) | ((tm == 0.0) & ~(hit & (t == 0.0)))}
        for what, m in classes.items():
            assert m.sum() >= 0.01 * c.n and m.sum() >= 1, (c.id, what, int(m.sum()))
        assert 0 < ref["occ_tmax"].sum() < hit.sum(), c.id


def test_a_write_back_moves_origins():
    cases = by_kind("writeback")
    assert cases
    for c in cases:
        r, moved = rays(c), reference(c)["moved"]
        changed = (r.view(np.int64) != moved.view(np.int64)).any(axis=1)
        assert changed.sum() >= 0.05 * c.n and changed.sum() >= 1, (c.id, int(changed.sum()))
        assert np.array_equal(r[:, 3:].view(np.int64), moved[:, 3:].view(np.int64))


def test_the_bounce_loop_still_has_rays_at_its_third_cast_and_has_retired_some():
    cases = by_kind("bounce")
    assert cases
    for c in cases:
        ref = reference(c)
        assert ref["events"].shape == (BOUNCES, c.n) and len(ref["per_cast"]) == BOUNCES
        assert 0 < ref["per_cast"][BOUNCES - 1]["rays"] < c.n, (c.id, ref["per_cast"])


def test_the_references_are_the_pinned_ones():
    with open(DIGESTS) as f:
        pinned = json.load(f)
    assert pinned == {c.id: digest(c) for c in CASES}
