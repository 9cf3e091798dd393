"""The receive loop's termination rules on the MI355X (include/hare_hip.h, "receivers", "Termination"): the time limit
(HARE_RECEIVE_TIME_LIMIT), the energy floor ("receive_floor_bits") and its roulette ("receive_roulette").  Every case of
tests.receive_cut_ref.cut_cases() -- each rule alone and all together, in the six kernel forms, on the three partitions, at batch sizes
about a wave, a workgroup and the live-block list's threshold, with bounce_pack and receive_aggregate on and off, from a starting state
with L past the end, infinities and NaN, and in an open room where rays also retire by missing -- through Receive_batch and, for a
subset, through receive_device on the caller's buffers.  Histogram, detections and final state (for the device call also the rays and
the last events) equal the numpy restatement (tests/receive_cut_ref.py) byte for byte; of a NaN only that it is one is compared.
tests/test_receive_cut_api.py proves with the restatement alone that the cases are not vacuous.  Further: the time-limit call's
histogram and binned detections are those of the call without the flag; the sharded call over two scenes equals the one-scene call
(the roulette draws on global ray indices); forty seeds of the receive sweep with the rules drawn on top."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests.receive_cases import mesh_of
from tests.receive_cut_ref import cut_cases, reference, same_bits, sweep_cut_case

pytestmark = pytest.mark.gpu

CASES = cut_cases()
SWEEP_SEEDS = 40


def library_partitions(cc, count=None):
    """The case's scene and partition in the library with receivers, tables and options set: `count` of them (default: case.shards)."""
    case = cc.case
    verts, nverts, _ = mesh_of(case.scene)
    T = H.Topology(verts, nverts)
    kind, *par = case.partition
    parts = []
    for _ in range(count or case.shards):
        p = H.Voxel_Grid([T], par[0]) if kind == "voxel" else (H.Octree if kind == "octree" else H.KDTree)([T], *par)
        p.set_receivers(case.centers, case.radii)
        if case.alpha is not None:
            p.set_absorption(case.alpha)
        if case.mode != "specular":
            p.set_scattering(case.sigma)
        p.set_option("scatter_seed", case.seed).set_option("bounce_pack", case.pack).set_option("receive_aggregate", case.aggregate)
        p.set_option("receive_floor_bits", cc.floor_bits).set_option("receive_roulette", int(cc.roulette))
        parts.append(p)
    return parts


def run_batch(cc, parts, time_limit=None):
    """Receive_batch (or the sharded call): (hist, detections, state)."""
    case = cc.case
    kw = dict(energy=case.state_in, frac_bits=case.frac_bits, poly_origin1=case.excl1, poly_origin2=case.excl2, rain=case.mode == "rain",
              directional=case.directional, time_limit=cc.time_limit if time_limit is None else time_limit)
    if len(parts) == 1:
        hist, _, det, state, _ = parts[0].Receive_batch(case.rays, case.bounces, case.n_bins, case.bin_len, **kw)
    else:
        hist, _, det, state, _ = type(parts[0]).Receive_batch_sharded(parts, case.rays, case.bounces, case.n_bins, case.bin_len, **kw)
    return hist, det, state


def run_device(cc, part):
    """receive_device on the caller's buffers, accumulators zeroed: dict of hist, det, state, rays, events."""
    import torch
    case = cc.case
    n, K, B = case.n, case.K, case.B
    rain = case.mode == "rain"
    state = case.state_in if case.state_in is not None else np.concatenate([np.zeros((1, n)), np.ones((B, n))])
    d_rays = torch.from_numpy(np.ascontiguousarray(case.rays)).to("cuda")
    d_state = torch.from_numpy(np.ascontiguousarray(state)).to("cuda")
    d_work = torch.zeros(H.Voxel_Grid.receive_work_bytes(n, rain), dtype=torch.uint8, device="cuda")
    d_last = torch.zeros(n * 56, dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros(case.words, dtype=torch.int64, device="cuda")
    d_det = torch.zeros(2 * K, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    part.receive_device(n, d_rays.data_ptr(), case.bounces, case.n_bins, case.bin_len, case.frac_bits, d_state.data_ptr(), d_work.data_ptr(),
                        d_last.data_ptr(), d_hist.data_ptr(), d_det.data_ptr(), rain=rain, directional=case.directional, time_limit=cc.time_limit)
    torch.cuda.synchronize()
    shape = (K, case.n_bins, B, 4) if case.directional else (K, case.n_bins, B)
    return dict(hist=d_hist.cpu().numpy().view(np.uint64).reshape(shape), det=d_det.cpu().numpy().view(np.uint64).reshape(K, 2),
                state=d_state.cpu().numpy(), rays=d_rays.cpu().numpy(),
                events=np.frombuffer(d_last.cpu().numpy().tobytes(), dtype=capi.XEVENT_DTYPE))


def mismatch(want, hist, det, state, rays=None, events=None):
    """The first difference between the library's results and the reference's, as text; None when there is none."""
    for what, got, ref in (("detections", det, want["det"]), ("histogram", hist, want["hist"]), ("state", state, want["state"])):
        bad = same_bits(got, ref)
        if bad:
            return f"{what}: {bad}"
    if rays is not None:
        bad = same_bits(rays, want["rays"])
        if bad:
            return f"rays: {bad}"
    if events is not None:
        for f in events.dtype.names:
            bad = same_bits(events[f], want["events"][f])
            if bad:
                return f"last X_Event.{f}: {bad}"
    return None


def check_case(cc, want, device=None):
    parts = library_partitions(cc)
    hist, det, state = run_batch(cc, parts)
    bad = mismatch(want, hist, det, state)
    if bad:
        return f"Receive_batch {bad}"
    if cc.case.device if device is None else device:
        got = run_device(cc, parts[0])
        bad = mismatch(want, got["hist"], got["det"], got["state"], got["rays"], got["events"])
        if bad:
            return f"receive_device {bad}"
    return None


@pytest.mark.parametrize("cc", CASES, ids=[c.name for c in CASES])
def test_case_equals_the_reference(cc):
    want = reference(cc)
    assert want["det"][:, 0].sum() > 0, cc.describe()
    bad = check_case(cc, want)
    assert bad is None, (cc.describe(), bad, {k: v.tolist() for k, v in want["per_cast"].items()})


@pytest.mark.parametrize("cc", [c for c in CASES if c.time_limit and c.case.n >= 4097], ids=lambda c: c.name)
def test_the_time_limit_changes_neither_histogram_nor_binned_detections_on_the_device(cc):
    parts = library_partitions(cc)
    h1, d1, s1 = run_batch(cc, parts, time_limit=True)
    h0, d0, s0 = run_batch(cc, parts, time_limit=False)
    assert h1.any()
    assert same_bits(h1, h0) is None and same_bits(d1[:, 0], d0[:, 0]) is None
    assert d1[:, 1].sum() < d0[:, 1].sum()              # the flag was not ignored: the retired rays' unbinned detections are gone
    assert same_bits(s1, s0) is not None


@pytest.mark.parametrize("cc", [c for c in CASES if c.name in ("roulette-4159", "all-4159", "all-state", "floor-4097")], ids=lambda c: c.name)
def test_two_scenes_on_one_device_equal_the_one_scene_call(cc):
    want = reference(cc)
    hist, det, state = run_batch(cc, library_partitions(cc, count=2))
    bad = mismatch(want, hist, det, state)
    assert bad is None, (cc.describe(), bad)


@pytest.mark.parametrize("seed", range(SWEEP_SEEDS))
def test_sweep_seed_with_the_rules_on_top_equals_the_reference(seed):
    cc = sweep_cut_case(seed)
    want = reference(cc, keep=False)
    bad = check_case(cc, want, device=seed % 4 == 0)
    print(cc.describe(), {k: int(v.sum()) for k, v in want["per_cast"].items()})
    assert bad is None, (cc.describe(), bad, {k: v.tolist() for k, v in want["per_cast"].items()})
