"""The receive loop on the MI355X at the numeric edges of its definition (include/hare_hip.h, "receivers"): every case of
tests.receive_cases.edge_cases() -- states full of NaN, infinities, negative values, signed zeros, denormals, ties and values that
saturate at 2^63 or clamp at +-2^62; sums that wrap; L exactly on a bin edge and at n_bins; B = 1 .. 8; K = 1, 64, 255, 256; batch
sizes about a wave, a workgroup and the live-block list's threshold; one bin, and a wave's lanes in distinct bins; exclusions on the
first cast; lanes whose arrival vector is not a number beside lanes that deposit -- through Receive_batch, and a subset through
receive_device with the caller's buffers.  Histogram, detections, final state (and, for the device call, rays and last events) equal
the numpy restatement (tests/receive_ref.py) byte for byte; of a NaN only that it is one is compared (its sign and payload are the FPU's,
DESIGN.md 1).  A directional call's channel 0, detections and state are those of the call without the flag.
tests/test_receive_cases.py proves, with the reference alone, that the cases hold these classes."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import capi
from tests.receive_cases import edge_cases, reference

pytestmark = pytest.mark.gpu

CASES = edge_cases()


def same_bits(got, want):
    """None when the two arrays agree: NaN where the other has NaN, and the same bits everywhere else.  Otherwise the first indices."""
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


def library_partitions(case, count=None):
    """The case's scene and partition in the library, with its receivers, tables and options set: `count` of them (default: case.shards)."""
    from tests.receive_cases import mesh_of
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
        parts.append(p)
    return parts


def run_batch(case, parts, directional=None):
    """Receive_batch (or the sharded call) on the case: (hist, detections, state)."""
    directional = case.directional if directional is None else directional
    kw = dict(energy=case.state_in, frac_bits=case.frac_bits, poly_origin1=case.excl1, poly_origin2=case.excl2, rain=case.mode == "rain",
              directional=directional)
    if len(parts) == 1:
        hist, _, det, state, _ = parts[0].Receive_batch(case.rays, case.bounces, case.n_bins, case.bin_len, **kw)
    else:
        hist, _, det, state, _ = type(parts[0]).Receive_batch_sharded(parts, case.rays, case.bounces, case.n_bins, case.bin_len, **kw)
    return hist, det, state


def run_device(case, part):
    """receive_device on the caller's buffers, accumulators zeroed: dict of hist, det, state, rays, events."""
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
    part.receive_device(n, d_rays.data_ptr(), case.bounces, case.n_bins, case.bin_len, case.frac_bits, d_state.data_ptr(), d_work.data_ptr(),
                        d_last.data_ptr(), d_hist.data_ptr(), d_det.data_ptr(), d_excl1=0 if d_e1 is None else d_e1.data_ptr(),
                        d_excl2=0 if d_e2 is None else d_e2.data_ptr(), rain=rain, directional=case.directional)
    torch.cuda.synchronize()
    shape = (K, case.n_bins, B, 4) if case.directional else (K, case.n_bins, B)
    return dict(hist=d_hist.cpu().numpy().view(np.uint64).reshape(shape), det=d_det.cpu().numpy().view(np.uint64).reshape(K, 2),
                state=d_state.cpu().numpy(), rays=d_rays.cpu().numpy(),
                events=np.frombuffer(d_last.cpu().numpy().tobytes(), dtype=capi.XEVENT_DTYPE))


def mismatch(case, want, hist, det, state, rays=None, events=None):
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


def check_case(case, want=None):
    """Runs the case through the library in every form it asks for; returns the first mismatch as text, or None."""
    want = want or reference(case)
    parts = library_partitions(case)
    hist, det, state = run_batch(case, parts)
    bad = mismatch(case, want, hist, det, state)
    if bad:
        return f"Receive_batch {bad}"
    if case.directional:                        # channel 0, detections and state are those of the call without the flag
        h0, d0, s0 = run_batch(case, parts, directional=False)
        bad = same_bits(h0, hist[..., 0]) or same_bits(d0, det) or same_bits(s0, state)
        if bad:
            return f"without the directional flag: {bad}"
    if case.device:
        got = run_device(case, parts[0])
        bad = mismatch(case, want, got["hist"], got["det"], got["state"], got["rays"], got["events"])
        if bad:
            return f"receive_device {bad}"
    return None


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_edge_case_equals_the_reference(case):
    want = reference(case)
    assert want["det"].sum() > 0, case.describe()
    bad = check_case(case, want)
    print(case.describe(), "tallies", {k: v for k, v in want["tallies"].items() if v})
    assert bad is None, (case.describe(), bad, {k: v for k, v in want["tallies"].items() if v})


def test_the_device_subset_holds_small_batches_and_the_threshold():
    ns = {c.n for c in CASES if c.device}
    assert any(n < 4096 for n in ns) and 4096 in ns and any(n < 256 for n in ns), ns
