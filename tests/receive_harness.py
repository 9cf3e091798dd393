"""The device side of the receive loop's differential tests (tests/test_gpu_receive_{edges,sweep,cut,map}.py, tools/fuzz_receive.py): a
tests.receive_cases.Case set up in the library, run through Receive_batch, the sharded call and receive_device, and compared with what
tests.receive_cases.reference returns for it -- byte for byte; of a NaN only that it is one (its sign and payload are the FPU's,
DESIGN.md 1).  torch and the GPU are touched in run_device alone: the module imports on a host without one."""
import numpy as np

import hare_amd as H
from hare_amd import capi
from tests.receive_cases import mesh_of

CALL_COUNTERS = ("hip_malloc_calls", "hip_free_calls", "hip_sync_calls")


def same_bits(got, want):
    """None when the two arrays agree: NaN where the other has NaN, the same bits everywhere else.  Otherwise the first differences,
    as text."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape / dtype {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        bad = (gn != wn) | (~gn & ~wn & (got.view(np.int64) != want.view(np.int64)))
    else:
        bad = got != want
    if bad.any():
        at = np.argwhere(bad)[:4]
        return f"{int(bad.sum())} differ, first at {at.tolist()}: got {[got[tuple(i)] for i in at]} want {[want[tuple(i)] for i in at]}"
    return None


def library_partitions(case, count=None, linear=False):
    """The case's scene and partition in the library with receivers, tables and options set: `count` of them (default: case.shards).
    linear: a map case's receivers through set_receivers."""
    verts, nverts, _ = mesh_of(case.scene)
    T = H.Topology(verts, nverts)
    kind, *par = case.partition
    parts = []
    for _ in range(count or case.shards):
        p = H.Voxel_Grid([T], par[0]) if kind == "voxel" else (H.Octree if kind == "octree" else H.KDTree)([T], *par)
        if case.map_cell is not None and not linear:
            p.set_receiver_map(case.centers, case.radii, case.map_cell)
        else:
            p.set_receivers(case.centers, case.radii)
        if case.alpha is not None:
            p.set_absorption(case.alpha)
        if case.sigma is not None:
            p.set_scattering(case.sigma)
        p.set_option("scatter_seed", case.seed).set_option("bounce_pack", case.pack).set_option("receive_aggregate", case.aggregate)
        p.set_option("receive_floor_bits", case.floor_bits).set_option("receive_roulette", int(case.roulette))
        parts.append(p)
    return parts


def run_batch(case, parts, **override):
    """Receive_batch (the sharded call for more than one partition) on the case, a keyword of the call overridden on request:
    (hist, detections, state)."""
    kw = dict(energy=case.state_in, frac_bits=case.frac_bits, poly_origin1=case.excl1, poly_origin2=case.excl2, rain=case.mode == "rain",
              directional=case.directional, time_limit=case.time_limit)
    kw.update(override)
    if len(parts) == 1:
        hist, _, det, state, _ = parts[0].Receive_batch(case.rays, case.bounces, case.n_bins, case.bin_len, **kw)
    else:
        hist, _, det, state, _ = type(parts[0]).Receive_batch_sharded(parts, case.rays, case.bounces, case.n_bins, case.bin_len, **kw)
    return hist, det, state


def run_device(case, part):
    """receive_device on the caller's buffers, accumulators zeroed: dict of hist, det, state, rays, events and calls, the change of
    CALL_COUNTERS over the call."""
    import torch
    n, K, B = case.n, case.K, case.B
    rain = case.mode == "rain"
    state = case.state_in if case.state_in is not None else np.concatenate([np.zeros((1, n)), np.ones((B, n))])
    d_rays = torch.from_numpy(np.ascontiguousarray(case.rays)).to("cuda")
    d_state = torch.from_numpy(np.ascontiguousarray(state)).to("cuda")
    d_work = torch.zeros(H.Voxel_Grid.receive_work_bytes(n, rain), dtype=torch.uint8, device="cuda")
    d_last = torch.zeros(n * 56, dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros(case.words, dtype=torch.int64, device="cuda")
    d_det = torch.zeros(2 * K, dtype=torch.int64, device="cuda")
    d_e1 = None if case.excl1 is None else torch.from_numpy(case.excl1).to("cuda")
    d_e2 = None if case.excl2 is None else torch.from_numpy(case.excl2).to("cuda")
    torch.cuda.synchronize()
    before = [part.get_option(o) for o in CALL_COUNTERS]
    part.receive_device(n, d_rays.data_ptr(), case.bounces, case.n_bins, case.bin_len, case.frac_bits, d_state.data_ptr(), d_work.data_ptr(),
                        d_last.data_ptr(), d_hist.data_ptr(), d_det.data_ptr(), d_excl1=0 if d_e1 is None else d_e1.data_ptr(),
                        d_excl2=0 if d_e2 is None else d_e2.data_ptr(), rain=rain, directional=case.directional, time_limit=case.time_limit)
    after = [part.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    shape = (K, case.n_bins, B, 4) if case.directional else (K, case.n_bins, B)
    return dict(hist=d_hist.cpu().numpy().view(np.uint64).reshape(shape), det=d_det.cpu().numpy().view(np.uint64).reshape(K, 2),
                state=d_state.cpu().numpy(), rays=d_rays.cpu().numpy(),
                events=np.frombuffer(d_last.cpu().numpy().tobytes(), dtype=capi.XEVENT_DTYPE),
                calls=[a - b for a, b in zip(after, before)])


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


def check_case(case, want, device=None, seen=None):
    """Runs the case through the library in every form it asks for (device: receive_device or not, whatever the case says); returns the
    first mismatch as text, or None.  seen: a dict that receives the partitions built ("parts") and, from a receive_device call, its
    "calls", or None."""
    parts = library_partitions(case)
    if seen is not None:
        seen["parts"] = parts
    hist, det, state = run_batch(case, parts)
    bad = mismatch(want, hist, det, state)
    if bad:
        return f"Receive_batch {bad}"
    if case.directional:                        # channel 0, detections and state are those of the call without the flag
        h0, d0, s0 = run_batch(case, parts, directional=False)
        bad = same_bits(h0, hist[..., 0]) or same_bits(d0, det) or same_bits(s0, state)
        if bad:
            return f"without the directional flag: {bad}"
    if case.device if device is None else device:
        got = run_device(case, parts[0])
        if seen is not None:
            seen["calls"] = got["calls"]
        bad = mismatch(want, got["hist"], got["det"], got["state"], got["rays"], got["events"])
        if bad:
            return f"receive_device {bad}"
    if case.two_scenes:
        hist, det, state = run_batch(case, library_partitions(case, count=2))
        bad = mismatch(want, hist, det, state)
        if bad:
            return f"Receive_batch_sharded {bad}"
    return None
