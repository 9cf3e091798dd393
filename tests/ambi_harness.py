"""The device side of the higher-order receivers' tests (tests/test_gpu_ambi*.py): a tests.ambi_cases.AmbiCase set up in the library
through tests.receive_harness, run through Receive_batch, the sharded call and receive_device at the case's order, and compared with
tests.ambi_cases.reference -- byte for byte, as tests.receive_harness compares.  torch and the GPU are touched in run_device alone."""
import numpy as np

import hare_amd as H
from hare_amd import capi
from tests import receive_harness as rh
from tests.receive_harness import library_partitions, mismatch, same_bits          # noqa: F401  (the tests take them from here)


def run_batch(case, parts, **override):
    """receive_harness.run_batch at the case's order (or the one overridden): (hist, detections, state)."""
    kw = dict(order=case.order)
    kw.update(override)
    return rh.run_batch(case, parts, **kw)


def run_device(case, part):
    """receive_device on the caller's buffers at the case's order, accumulators zeroed: dict of hist, det, state, rays, events, calls."""
    import torch
    n, K, B = case.n, case.K, case.B
    rain = case.mode == "rain"
    state = case.state_in if case.state_in is not None else np.concatenate([np.zeros((1, n)), np.ones((B, n))])
    d_rays = torch.from_numpy(np.ascontiguousarray(case.rays)).to("cuda")
    d_state = torch.from_numpy(np.ascontiguousarray(state)).to("cuda")
    d_work = torch.zeros(H.Voxel_Grid.receive_work_bytes(n, rain), dtype=torch.uint8, device="cuda")
    d_last = torch.zeros(n * 56, dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros(case.words + 64, dtype=torch.int64, device="cuda")                   # 64 guard words behind the histogram
    d_det = torch.zeros(2 * K, dtype=torch.int64, device="cuda")
    d_e1 = None if case.excl1 is None else torch.from_numpy(case.excl1).to("cuda")
    d_e2 = None if case.excl2 is None else torch.from_numpy(case.excl2).to("cuda")
    torch.cuda.synchronize()
    before = [part.get_option(o) for o in rh.CALL_COUNTERS]
    part.receive_device(n, d_rays.data_ptr(), case.bounces, case.n_bins, case.bin_len, case.frac_bits, d_state.data_ptr(), d_work.data_ptr(),
                        d_last.data_ptr(), d_hist.data_ptr(), d_det.data_ptr(), d_excl1=0 if d_e1 is None else d_e1.data_ptr(),
                        d_excl2=0 if d_e2 is None else d_e2.data_ptr(), rain=rain, directional=True, time_limit=case.time_limit, order=case.order)
    after = [part.get_option(o) for o in rh.CALL_COUNTERS]
    torch.cuda.synchronize()
    words = d_hist.cpu().numpy().view(np.uint64)
    assert not words[case.words:].any(), "words behind the histogram were written"
    return dict(hist=words[:case.words].reshape(K, case.n_bins, B, case.channels), det=d_det.cpu().numpy().view(np.uint64).reshape(K, 2),
                state=d_state.cpu().numpy(), rays=d_rays.cpu().numpy(),
                events=np.frombuffer(d_last.cpu().numpy().tobytes(), dtype=capi.XEVENT_DTYPE),
                calls=[a - b for a, b in zip(after, before)])


def check_case(case, want, device=None, lower=True):
    """The case through the library in every form it asks for; the first mismatch as text, or None.  lower: also that the call one
    order down (and the first-order call) returns this call's leading channels, and the same detections and state."""
    parts = library_partitions(case)
    hist, det, state = run_batch(case, parts)
    bad = mismatch(want, hist, det, state)
    if bad:
        return f"Receive_batch {bad}"
    if lower:
        for order in range(1, case.order):
            h, d, s = run_batch(case, parts, order=order)
            bad = same_bits(h, hist[..., :h.shape[3]]) or same_bits(d, det) or same_bits(s, state)
            if bad:
                return f"order {order} against the head of order {case.order}: {bad}"
    if case.device if device is None else device:
        got = run_device(case, parts[0])
        bad = mismatch(want, got["hist"], got["det"], got["state"], got["rays"], got["events"])
        if bad:
            return f"receive_device {bad}"
        if got["calls"] != [0, 0, 0]:
            return f"receive_device made runtime calls: {got['calls']}"
    if case.shards > 1 or case.two_scenes:
        hist, det, state = run_batch(case, library_partitions(case, count=2))
        bad = mismatch(want, hist, det, state)
        if bad:
            return f"Receive_batch_sharded {bad}"
    return None
