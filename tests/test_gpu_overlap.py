"""K1q's fused round (hare_amd/csrc/voxel_pool.hip; scene option `voxel_overlap`): a bulk round whose cull queue AND walk queue are worth
a task runs both -- the cull task's list entries are requested, the walk task's step loops run while they are in flight, the cull
consumes them.  No load is added, per ray the operations and their order stay what they were, so every X_Event must be the same bytes:
each case runs with the option on, off and through the oracle, all eight fields bit-equal.  The cases: the bench's shapes (the hall at
D = 64 -- a bit per voxel -- with 1 048 576 rays, the cathedral at D = 128 -- a bit per 2^3 block -- with 2 097 152), quadrilaterals,
both exclusions, origins outside the grid with and without the origin write-back, batches from one ray to 262 144, the bounce loop
cast by cast both ways, and the counting build's own-work counters."""
import numpy as np
import pytest

import hare_amd as H
from oracle import pyoracle as po
from tests.helpers import assert_events_equal, oracle_bounce_loop

pytestmark = pytest.mark.gpu


def on_off(g, rays, ref, what, hits=None, **kw):
    for ov in (1, 0):
        g.set_option("voxel_overlap", ov)
        assert g.get_option("voxel_overlap") == ov
        # the option chooses the kernel: the builds with the fused round are kernels of their own (hare_voxel_pool_*_ov)
        assert g.kernel_name(len(rays)).endswith("_ov") == (ov == 1), (ov, g.kernel_name(len(rays)))
        ev, c = g.Shoot_batch(rays, **kw)
        assert_events_equal(ev, ref, what=f"{what} voxel_overlap={ov}")
        if hits is not None:
            assert c["hits"] == hits
    g.set_option("voxel_overlap", 0)


def scene_pair(scene, domain):
    m = H.scenes.SCENES[scene]()
    T, To = H.Topology(m.verts, m.nverts), po.Topology(m.verts, m.nverts)
    return m, To, H.Voxel_Grid([T], domain), po.VoxelGrid([To], domain=domain)


def test_option_defaults_to_off():
    """The fused round is slower on the headline, so one phase per round stays the default."""
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    assert g.get_option("voxel_overlap") == 0


@pytest.mark.parametrize("scene,domain,n", [("hall", 64, 1 << 20), ("cathedral", 128, 2 << 20), ("hall_quads", 64, 1 << 20)])
def test_fused_round_at_bench_shapes(scene, domain, n):
    m, To, g, o = scene_pair(scene, domain)
    rays = H.scenes.burst_rays(n, m.size)
    assert g.kernel_name(n).startswith("hare_voxel_pool"), g.kernel_name(n)
    ref, rc = o.shoot(rays, nthreads=32)
    on_off(g, rays, ref, f"{scene} D={domain}", hits=rc["hits"])


@pytest.mark.parametrize("k", [1, 63, 64, 65, 4097, 262_144])
def test_fused_round_batch_sizes(k):
    m, To, g, o = scene_pair("hall", 64)
    rays = H.scenes.burst_rays(1 << 20, m.size)[:: (1 << 20) // k][:k].copy()         # k rays spread over the whole burst
    assert len(rays) == k
    ref, rc = o.shoot(rays, nthreads=16)
    on_off(g, rays, ref, f"hall D=64 {k} rays", hits=rc["hits"])


@pytest.mark.parametrize("scene,domain", [("hall", 64), ("cathedral", 128)])
def test_fused_round_with_exclusions(scene, domain):
    m, To, g, o = scene_pair(scene, domain)
    n = 300_000
    rays = H.scenes.burst_rays(n, m.size)
    first, _ = o.shoot(rays, nthreads=16)
    rng = np.random.default_rng(7)
    np_ = len(m.nverts)
    e1 = np.where(rng.random(n) < 0.6, first["poly_id"], rng.integers(-1, np_, n)).astype(np.int32)
    e2 = rng.integers(-1, np_, n).astype(np.int32)
    ref1, rc1 = o.shoot(rays, excl1=e1, nthreads=16)
    on_off(g, rays, ref1, f"{scene} excl1", hits=rc1["hits"], poly_origin1=e1)
    ref2, rc2 = o.shoot(rays, excl1=e1, excl2=e2, nthreads=16)
    on_off(g, rays, ref2, f"{scene} excl1+excl2", hits=rc2["hits"], poly_origin1=e1, poly_origin2=e2)


@pytest.mark.parametrize("scene,domain", [("hall", 64), ("cathedral", 128)])
def test_fused_round_with_origins_outside_the_grid(scene, domain):
    """A ray whose origin AABB.Intersect moved keeps t_start in its event slot; the cull reads it (F_MOVED) unless the origin is written back."""
    m, To, g, o = scene_pair(scene, domain)
    n = 300_000
    rays = H.scenes.burst_rays(n, m.size)
    rays[::2, :3] -= rays[::2, 3:] * (2.0 * float(max(m.size)))          # every other ray starts far outside, looking in
    rays[1::7, :3] += 3.0 * float(max(m.size))                            # ... some of the rest outside, looking wherever they look
    ref, rc = o.shoot(rays, nthreads=16)
    assert 0 < rc["hits"] < n
    on_off(g, rays, ref, f"{scene} outside origins", hits=rc["hits"])
    refm, _, moved = o.shoot(rays, mutate=True)
    for ov in (1, 0):
        g.set_option("voxel_overlap", ov)
        r = rays.copy()
        ev, _ = g.Shoot_batch(r, writeback_origin=True)
        assert_events_equal(ev, refm, what=f"{scene} outside origins, write-back, voxel_overlap={ov}")
        assert np.array_equal(r.view(np.int64), moved.view(np.int64))
    g.set_option("voxel_overlap", 0)


@pytest.mark.parametrize("scene,domain,n", [("hall", 64, 120_000), ("cathedral", 128, 60_000)])
def test_fused_round_in_the_bounce_loop(scene, domain, n):
    """Eight casts, cast by cast against the oracle's loop: a launch per cast (the pool kernel, fused rounds) and the one-launch loop."""
    m, To, g, o = scene_pair(scene, domain)
    rays = H.scenes.burst_rays(n, m.size)
    ref, rc = oracle_bounce_loop(po, To, o, rays, 8)
    for ov in (1, 0):
        g.set_option("voxel_overlap", ov)
        for fused in (0, 1):
            g.set_option("bounce_fused", fused)
            ev, c, pcs = g.Bounce_batch(rays, 8, per_cast=True, all_casts=True)
            for b in range(8):
                assert_events_equal(ev[b], ref[b], what=f"{scene} bounce cast {b} voxel_overlap={ov} bounce_fused={fused}")
            assert [(p["rays"], p["hits"]) for p in pcs] == [(p["rays"], p["hits"]) for p in rc]
    g.set_option("bounce_fused", 0); g.set_option("voxel_overlap", 0)


def test_own_work_counters_do_not_depend_on_the_fused_round():
    """HARE_SHOOT_COUNT_OWN: voxels walked into, list entries scanned, candidates pre-culled, exact tests made (C', L', K', T') do not
    depend on the option, and every event is the same bytes.  There is no counting build with the fused round (registers,
    voxel_pool.hip): the option must leave the counting kernel's choice alone, which is what this pins -- as
    test_own_work_counters_do_not_depend_on_the_step_loop does for the step loop, with its bound (two launches draw their tickets
    differently, and a ray the drain's wide modes pick up re-scans its voxel's list)."""
    import torch
    from hare_amd import capi
    for scene, D in (("hall", 64), ("cathedral", 128)):
        m = H.scenes.SCENES[scene]()
        g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], D)
        n = 300_000
        d_rays = torch.from_numpy(H.scenes.burst_rays(n, m.size)).cuda()
        d_out = torch.empty(n * 56, dtype=torch.uint8, device="cuda")
        got = {}
        for ov in (1, 0):
            g.set_option("voxel_overlap", ov)
            d_ctr = torch.zeros(8, dtype=torch.int64, device="cuda")
            assert g.kernel_name(n, flags=capi.SHOOT_COUNT_OWN).endswith("_own")
            assert g.kernel_name(n).endswith("_ov") == (ov == 1)
            g.shoot_device(n, d_rays.data_ptr(), d_out.data_ptr(), d_counters=d_ctr.data_ptr(), flags=capi.SHOOT_COUNT_OWN)
            torch.cuda.synchronize()
            got[ov] = (d_out.cpu().numpy().tobytes(), [int(x) for x in d_ctr.cpu()])
        g.set_option("voxel_overlap", 0)
        assert got[1][0] == got[0][0], scene
        # the same rays and hits; the work counters agree to within what the drain makes of two launches' different ticket draws (a ray the
        # cooperative tail or a wide mode picks up re-scans its voxel's list): the bound of the step loop's test, well under 2 %
        a, b = got[1][1], got[0][1]
        assert a[:2] == b[:2] == [n, a[1]], (scene, a, b)
        for k in (2, 3, 4, 5):
            assert abs(a[k] - b[k]) <= 0.02 * b[k], (scene, a, b)
