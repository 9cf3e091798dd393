"""The GPU partition builders (build_gpu.cpp, build_kernels.hip) on the MI355X at the sizes where they take another path: the cases of
tests.build_cases.edge_cases(), which tests/test_build_cases.py shows to reach those sizes on the oracle alone.  Per case, built with the
device builders: `built_on_device` (0 only for the octree of several topologies, which is the host builder's), lists or node arrays, `ct`,
`total_items`, boxes and voxel dimensions equal to the oracle's, and a second build of the same case equal to the first byte for byte
(the fixed grid's fill is atomic; only the sort makes it deterministic).  hare_vb_finalize's cell records and occupancy bits,
hare_cell_boxes and hare_block_occ have no read-back: they are checked through shoots -- rays half of which are aimed at the clusters,
with "voxel_tight" and "voxel_skip" 0 and 1, against the oracle's events bit for bit, and through a host-built grid of the same scene as
well.  All comparisons are equalities."""
import numpy as np
import pytest

from tests import build_cases as bc
from tests.helpers import assert_events_equal

pytestmark = pytest.mark.gpu

EDGES = {c.name: c for c in bc.edge_cases()}


@pytest.fixture(autouse=True)
def device_builders(monkeypatch):
    monkeypatch.delenv("HARE_BUILD", raising=False)


def arrays_of(case, part):
    return list(part.nodes()) if case.kind == "octree" else [a for m in range(len(case.topos)) for a in part.Voxel_Inv(m)]


@pytest.mark.parametrize("name", list(EDGES))
def test_device_builder_equals_the_oracle_and_itself(name):
    case = EDGES[name]
    ref = bc.reference(case, keep=True)
    part = bc.build(case)
    assert part.info().built_on_device == (0 if case.kind == "octree" and len(case.topos) > 1 else 1), case.describe()
    bad = bc.compare(case, part, ref)
    assert bad is None, (case.describe(), bad)
    again = bc.build(case)
    for a, b in zip(arrays_of(case, part), arrays_of(case, again)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), case.describe()


def shoot_all_ways(case, part, ref, rays, what):
    """The grid's shoots with the voxels' tight boxes and the block occupancy off and on, every topology, against the oracle's events."""
    for top in range(len(case.topos)):
        want, wc = ref["oracle"].shoot(rays, top, nthreads=16)
        assert 0 < want["hit"].sum()
        for tight in (0, 1):
            for skip in (0, 1):
                part.set_option("voxel_tight", tight)
                part.set_option("voxel_skip", skip)
                ev, c = part.Shoot_batch(rays, top)
                assert_events_equal(ev, want, what=f"{what} top {top} voxel_tight={tight} voxel_skip={skip}")
                assert c["hits"] == wc["hits"]


@pytest.mark.parametrize("name", [n for n, c in EDGES.items() if c.shoot])
def test_cell_records_occupancy_and_tight_boxes_through_shoots(name):
    case = EDGES[name]
    ref = bc.reference(case, keep=True)
    rays = bc.rays_for(case)
    part = bc.build(case)
    assert part.info().built_on_device == 1
    shoot_all_ways(case, part, ref, rays, name + " device-built")
    host = bc.build(case, host=True)
    assert host.info().built_on_device == 0
    shoot_all_ways(case, host, ref, rays, name + " host-built")


def test_rebuild_on_one_scene_handle():
    """A scene that holds a device grid is built again -- fixed D = 4, fixed D = 13, adaptive, fixed D = 4 --: the old buffers are replaced,
    the tight boxes and the block occupancy uploaded again.  After each build the lists equal the oracle's and a fresh scene's, and a shoot
    equals the oracle's."""
    base = EDGES["lengths-D4"]
    rays = bc.rays_for(base)
    part = None
    for builder in (("fixed", 4), ("fixed", 13), ("adaptive", 4, 1000), ("fixed", 4)):
        case = bc.BuildCase("rebuild " + " ".join(str(x) for x in builder), base.topos, builder, aim=base.aim)
        ref = bc.reference(case)
        if part is None:
            part = bc.build(case)
            part.set_option("voxel_skip", 1)
        else:
            bc.rebuild(part, builder)
        assert part.info().built_on_device == 1
        bad = bc.compare(case, part, ref)
        assert bad is None, (case.describe(), bad)
        fresh = bc.build(case)
        for a, b in zip(arrays_of(case, part), arrays_of(case, fresh)):
            assert a.tobytes() == b.tobytes(), case.describe()
        want, _ = ref["oracle"].shoot(rays, nthreads=16)
        for skip in (1, 0, 1):
            part.set_option("voxel_skip", skip)
            assert_events_equal(part.Shoot_batch(rays)[0], want, what=f"{case.name} voxel_skip={skip}")
        assert_events_equal(fresh.Shoot_batch(rays)[0], want, what=f"{case.name} fresh scene")
