"""The voxel kernels under every pair of their switches, call modes and shapes (tests/voxel_cases.py): K1q and its builds, K1p, the
occlusion kernels and the bounce loop on scenes of a few hundred polygons with at most 8 193 rays, every case against the oracle on all
eight X_Event fields by bit pattern, with the counters, the flags and the moved origins the mode returns.  The first thing to run after a
change to voxel_pool.hip: a case's id names every option that is not at its first level."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests.helpers import FIELDS, assert_events_equal
from tests.receive_harness import CALL_COUNTERS
from tests.voxel_cases import BOUNCES, CASES, DEFAULTS, FACTORS, FAMILIES, NAMES, Case, grid_args, rays, reference, scene

pytestmark = pytest.mark.gpu

GUARD = 64                                            # words behind every output of a device call that must stay as they were
POISON = 0x5A5A5A5A5A5A5A5A
_GRIDS = {}


def grid_of(case):
    """the case's grid, built once per (scene, grid); every case leaves it with the options it was created with"""
    key = (case.scene, case.grid)
    if key not in _GRIDS:
        tops, _, _ = scene(case)
        D, avg = grid_args(case.grid)
        _GRIDS[key] = H.Voxel_Grid([H.Topology(v, nv) for v, nv in tops], D, avg)
        assert {k: _GRIDS[key].get_option(k) for k in DEFAULTS} == DEFAULTS
    return _GRIDS[key]


class options:
    """the case's options set and read back; the defaults put back on the way out"""

    def __init__(self, g, case):
        self.g, self.case = g, case

    def __enter__(self):
        for k, v in self.case.options.items():
            self.g.set_option(k, v)
            assert self.g.get_option(k) == v, k
        return self.g

    def __exit__(self, *exc):
        for k, v in DEFAULTS.items():
            self.g.set_option(k, v)
        return False


def device_shoot(g, top, r, e1, flags, poison=POISON):
    """hare_shoot_device on torch tensors: (events, counter words, guards untouched, change of CALL_COUNTERS over the call)"""
    import torch
    n = len(r)
    d_rays = torch.from_numpy(np.array(r)).to("cuda")
    d_e1 = None if e1 is None else torch.from_numpy(np.array(e1)).to("cuda")
    d_out = torch.full((n * 7 + GUARD,), poison, dtype=torch.int64, device="cuda")
    d_ctr = torch.full((8 + GUARD,), poison, dtype=torch.int64, device="cuda")
    d_ctr[:8] = 0
    torch.cuda.synchronize()
    before = [g.get_option(o) for o in CALL_COUNTERS]
    g.shoot_device(n, d_rays.data_ptr(), d_out.data_ptr(), top_index=top, d_excl1=0 if d_e1 is None else d_e1.data_ptr(),
                   d_counters=d_ctr.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, flags=flags)
    after = [g.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    out, ctr = d_out.cpu().numpy(), d_ctr.cpu().numpy()
    intact = bool((out[n * 7:] == poison).all() and (ctr[8:] == poison).all() and d_rays.cpu().numpy().tobytes() == r.tobytes())
    return np.frombuffer(out[:n * 7].tobytes(), dtype=capi.XEVENT_DTYPE), [int(x) for x in ctr[:8]], intact, [a - b for a, b in zip(after, before)]


def run(g, case, poison=POISON):
    """The case's mode on a grid that has its options: (events as the mode returns them, a dict of what else it returned)."""
    ref, r = reference(case), rays(case)
    top = scene(case)[1]
    mode = case.mode
    if mode == "closest":
        ev, c = g.Shoot_batch(r, top_index=top)
    elif mode == "excl":
        ev, c = g.Shoot_batch(r, top_index=top, poly_origin1=ref["e1"], poly_origin2=ref["e2"])
    elif mode == "writeback":
        mine = np.array(r)
        ev, c = g.Shoot_batch(mine, top_index=top, writeback_origin=True)
        return ev, dict(c, moved=mine)
    elif mode == "slim":
        sl, c = g.Shoot_batch(r, top_index=top, slim=True)
        assert sl.dtype == capi.SLIM_DTYPE
        ev = g.expand_events(r, sl)
    elif mode in ("retired", "own"):
        flags = capi.SHOOT_RETIRED_RAYS if mode == "retired" else capi.SHOOT_COUNT_OWN
        ev, w, intact, calls = device_shoot(g, top, r, ref["e1"], flags, poison)
        return ev, dict(rays=w[0], hits=w[1], entries=w[3], culls=w[5], intact=intact, calls=calls)
    elif mode in ("occl", "occl_tmax"):
        occ, c = g.Occluded_batch(r, ref["tmax"] if mode == "occl_tmax" else None, top_index=top, events=False)
        return None, dict(c, occ=occ)
    else:
        ev, c, per_cast = g.Bounce_batch(r, BOUNCES, top_index=top, per_cast=True, all_casts=True)
        last, c2, per_cast2 = g.Bounce_batch(r, BOUNCES, top_index=top, per_cast=True)      # one event buffer: retired rays are not written again
        return ev, dict(c, per_cast=per_cast, last=last, rays2=c2["rays"], hits2=c2["hits"], per_cast2=per_cast2)
    return ev, c


def same_bits(a, b, what):
    """all eight fields by bit pattern (assert_events_equal compares values: it says which rays differ, this that -0.0 is not 0.0)"""
    assert_events_equal(a, b, what=what)
    for f in FIELDS:
        assert np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes(), f"{what} X_Event.{f} differs in its bits"


def check(case, ev, got):
    ref = reference(case)
    what = case.id
    if case.mode in ("occl", "occl_tmax"):
        want = ref["occ_tmax"] if case.mode == "occl_tmax" else ref["occ_any"]
        assert got["occ"].dtype == np.int32
        bad = np.nonzero(got["occ"] != want)[0]
        assert bad.size == 0, (what, bad[:5], ref["plain"][bad[:5]])
        assert got["rays"] == case.n and got["hits"] == int(want.sum()), what          # hits of a flags-only call: the occluded rays
        return
    if case.mode == "bounce":
        for b in range(BOUNCES):
            same_bits(ev[b], ref["events"][b], f"{what} cast {b}")
        want = [(p["rays"], p["hits"]) for p in ref["per_cast"]]
        assert [(p["rays"], p["hits"]) for p in got["per_cast"]] == want and [(p["rays"], p["hits"]) for p in got["per_cast2"]] == want, what
        same_bits(got["last"], ref["events"][BOUNCES - 1], f"{what} last cast only")
        assert (got["rays2"], got["hits2"]) == (ref["rays"], ref["hits"]), what
    else:
        same_bits(ev, ref["events"], what)
    assert got["rays"] == ref["rays"] and got["hits"] == ref["hits"], (what, got["rays"], got["hits"], ref["rays"], ref["hits"])
    if case.mode == "writeback":
        mine, moved = got["moved"], ref["moved"]
        ok = ~np.isnan(moved).any(axis=1)   # NaN payload bits of a moved NaN origin are not part of the contract
        assert np.array_equal(mine[ok].view(np.int64), moved[ok].view(np.int64)), what
        assert np.array_equal(np.isnan(mine), np.isnan(moved)), what
    if case.mode in ("retired", "own"):
        assert got["intact"], what          # nothing behind the events or the counters, nothing in the rays
        assert got["calls"] == [0, 0, 0], (what, got["calls"])
    if case.mode == "own":                  # what the counting build did: every pre-culled candidate is a list entry scanned
        assert got["culls"] <= got["entries"], (what, got)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_every_case_equals_the_oracle_bit_for_bit(case):
    with options(grid_of(case), case) as g:
        ev, got = run(g, case)
    check(case, ev, got)
    assert {k: grid_of(case).get_option(k) for k in DEFAULTS} == DEFAULTS


def test_the_cases_launch_every_kernel_of_the_voxel_table():
    """The names hare_shoot_kernel_name gives for the cases, with their options set, hold every member of the families Pool, PoolOv, PoolOwn
    and Persist in device_scene.cpp's table (read by regex: a new member fails here until a case reaches it), and those of Bounce.
    hare_shoot_kernel_name cannot name the occlusion build (its flags do not say "no events"), so for Occl the other way is taken: the
    list holds an occlusion case in each cell {fine, coarse bitmap} x {triangles, quadrilaterals}; that the cell is the grid's is read
    from the Pool name of the same grid."""
    import os
    import re
    from tests.voxel_cases import ROOT
    src = open(os.path.join(ROOT, "hare_amd", "csrc", "device_scene.cpp")).read()
    table = re.search(r"kVoxelKernelNames\[DeviceModule::kFamilies\]\[2\]\[2\] = \{(.*?)\n\};", src, re.S).group(1)
    rows = [re.findall(r'"(hare_voxel_\w+)"', line) for line in table.strip().split("\n")]
    assert len(rows) == len(FAMILIES) and all(len(r) == 4 for r in rows)
    by_family = dict(zip(FAMILIES, rows))
    launched, occl_cells = set(), set()
    for case in CASES:
        top = scene(case)[1]
        with options(grid_of(case), case) as g:
            flags = {"own": capi.SHOOT_COUNT_OWN, "bounce": capi.SHOOT_BOUNCE_LOOP}.get(case.mode, 0)
            name = g.kernel_name(case.n, top, flags)
            if case.mode in ("occl", "occl_tmax"):
                g.set_option("voxel_kernel", 2); g.set_option("voxel_overlap", 0)
                occl_cells.add(by_family["Pool"].index(g.kernel_name(case.n, top)))
            else:
                launched.add(name)
                if case.mode == "bounce":                      # the loop of a launch per cast runs the shoot's own kernel
                    launched.add(g.kernel_name(case.n, top, capi.SHOOT_RETIRED_RAYS))
    for fam in ("Pool", "PoolOv", "PoolOwn", "Persist", "Bounce"):
        assert set(by_family[fam]) <= launched, (fam, sorted(set(by_family[fam]) - launched))
    assert occl_cells == {0, 1, 2, 3}


def test_two_runs_give_the_same_bytes_whatever_the_outputs_held():
    """The order pass places a window's rays by LDS atomics and the wide drain hands rays between lanes: neither may show in the events.  A
    device call with voxel_order = 2 and wide_drain = 1 into outputs poisoned with 0 and with 0x5A..."""
    case = Case(len(CASES), **dict({k: FACTORS[k][0] for k in NAMES}, scene="soup", grid="D33", rays="awkward", n=FACTORS["n"][-1], mode="retired",
                                   voxel_order=2, wide_drain=1))
    with options(grid_of(case), case) as g:
        a, ga = run(g, case, poison=0)
        b, gb = run(g, case, poison=POISON)
    assert a.tobytes() == b.tobytes() and (ga["rays"], ga["hits"]) == (gb["rays"], gb["hits"])
    check(case, a, ga)
