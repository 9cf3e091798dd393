"""The device side of the source paths' differential tests (tests/test_gpu_path_{edges,sweep,ambi}.py, tools/fuzz_paths.py): a
tests.path_cases.PathCase set up in the library and run through direct_device, Image_device and Image2_device for the orders it names, at
the ambisonic order it names (one, four, nine or sixteen channels: every size here follows from case.shape) --
onto random non-zero words, with guard bytes behind every buffer and lists of exactly the counts the reference found -- and compared with
what tests.path_cases.reference returns for it.  torch and the GPU are touched in check_case alone: the module imports on a host without
one."""
import numpy as np

import hare_amd as H
from tests.receive_harness import CALL_COUNTERS

GUARD = 64                                   # bytes behind d_work; 8-byte words behind d_hist and d_detections
FILL = 0xA5


def library_partition(case):
    """The case's mesh and partition in the library with receivers, tables, source and options set: (partition, topology)."""
    T = H.Topology(case.verts, case.nverts)
    kind, *par = case.partition
    g = H.Voxel_Grid([T], par[0]) if kind == "voxel" else (H.Octree if kind == "octree" else H.KDTree)([T], *par)
    (g.set_receiver_map if case.map else g.set_receivers)(case.centers, case.radii)
    if case.alpha is not None:
        g.set_absorption(case.alpha)
    elif case.B > 1:
        g.set_absorption(np.zeros((case.P, case.B)))                   # fixes the topology's B
    if case.sigma is not None:
        g.set_scattering(case.sigma)
    g.set_source(case.pos, power=case.power, frame=case.frame, gain=case.gain)
    g.set_option("image_cull", case.image_cull).set_option("image2_prune", case.image2_prune)
    return g, T


def run_order(torch, g, case, order, work_bytes, call):
    """One device call of the case onto random words: (added histogram, added detections, the work array) or the text of what it
    touched that it must not."""
    K, words = case.K, int(np.prod(case.shape))
    rng = np.random.default_rng(3)
    base_h = rng.integers(0, 2 ** 64, words + GUARD, dtype=np.uint64)           # the calls ACCUMULATE: onto words that are not zero
    base_d = rng.integers(0, 2 ** 64, 2 * K + GUARD, dtype=np.uint64)
    d_hist = torch.from_numpy(base_h.view(np.int64)).to("cuda")
    d_det = torch.from_numpy(base_d.view(np.int64)).to("cuda")
    d_work = torch.full((work_bytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = [g.get_option(o) for o in CALL_COUNTERS]
    call(d_work.data_ptr(), d_hist.data_ptr(), d_det.data_ptr())
    after = [g.get_option(o) for o in CALL_COUNTERS]
    torch.cuda.synchronize()
    if after != before:
        return f"{order}: HIP call counters moved: {dict(zip(CALL_COUNTERS, (a - b for a, b in zip(after, before))))}"
    hist, det, work = d_hist.cpu().numpy().view(np.uint64), d_det.cpu().numpy().view(np.uint64), d_work.cpu().numpy()
    if not ((work[work_bytes:] == FILL).all() and (hist[words:] == base_h[words:]).all() and (det[2 * K:] == base_d[2 * K:]).all()):
        return f"{order}: guard bytes touched"
    with np.errstate(over="ignore"):
        return (hist[:words] - base_h[:words]).reshape(case.shape), (det[:2 * K] - base_d[:2 * K]).reshape(K, 2), work


def differ(order, got_h, got_d, want):
    bad = np.argwhere(got_d != want["det"])
    if bad.size:
        return f"{order} detections: {len(bad)} differ, first at {bad[:4].tolist()}: got {got_d[tuple(bad[0])]} want {want['det'][tuple(bad[0])]}"
    bad = np.argwhere(got_h != want["hist"])
    if bad.size:
        return f"{order} histogram: {len(bad)} differ, first at {bad[:4].tolist()}: got {got_h[tuple(bad[0])]} want {want['hist'][tuple(bad[0])]}"
    return None


def check_case(case, want):
    """Runs the case's orders on the device; returns the first difference from `want` (tests.path_cases.reference of the case) as text,
    or None.  Histogram and detections byte for byte; the counts; the pair list as a set; the candidate list as a set -- equal with the
    prune off, a superset of every reference path's (p, q) with it on --; the guards; the HIP call counters."""
    import torch
    g, T = library_partition(case)
    P, K = case.P, case.K
    tail = (case.n_weight, case.n_bins, case.bin_len, case.frac_bits)
    for order in case.orders:
        w = want[order]
        if order == "direct":
            got = run_order(torch, g, case, order, H.Voxel_Grid.direct_work_bytes(K),
                            lambda dw, dh, dd: g.direct_device(*tail, dw, dh, dd, directional=case.directional, order=case.order))
            if isinstance(got, str):
                return got
        elif order == "image":
            M = max(1, w["pairs"])                                      # a list of exactly the pairs there are
            got = run_order(torch, g, case, order, H.Voxel_Grid.image_work_bytes(K, P, M),
                            lambda dw, dh, dd: g.Image_device(*tail, M, dw, dh, dd, directional=case.directional, order=case.order))
            if isinstance(got, str):
                return got
            work = got[2]
            found = int(work[:8].view(np.uint64)[0])
            if found != w["pairs"]:
                return f"image: {found} pairs found, want {w['pairs']}"
            kp = work[256 + 32 * P + 112 * M:][:8 * M].view(np.int32).reshape(M, 2)[:found]      # behind the shadow rays and their t_max
            s = w["seen"]
            if sorted(map(tuple, kp.tolist())) != sorted(zip(s["k"].tolist(), s["p"].tolist())):
                return f"image: the pair list differs: {sorted(set(map(tuple, kp.tolist())) ^ set(zip(s['k'].tolist(), s['p'].tolist())))[:4]}"
        else:
            C, M = max(1, w["cands"]), max(1, w["paths"])
            got = run_order(torch, g, case, order, H.Voxel_Grid.image2_work_bytes(P, C, M),
                            lambda dw, dh, dd: g.Image2_device(*tail, C, M, dw, dh, dd, directional=case.directional, order=case.order))
            if isinstance(got, str):
                return got
            work = got[2]
            nc, m = (int(x) for x in work[:16].view(np.uint64))
            if m != w["paths"] or (nc > w["cands"] if case.image2_prune else nc != w["cands"]):
                return f"image2: {nc} candidates and {m} paths found, want {w['cands']} and {w['paths']}"
            pq = set(map(tuple, work[256 + 32 * P + 24 * C:][:8 * C].view(np.int32).reshape(C, 2)[:nc].tolist()))      # behind the images and S''
            if len(pq) != nc:
                return "image2: a candidate is listed twice"
            s = w["seen"]
            cd = s["cands"]
            every, need = set(zip(cd["p"].tolist(), cd["q"].tolist())), set(zip(s["p"].tolist(), s["q"].tolist()))
            if not (need <= pq <= every) or (not case.image2_prune and pq != every):
                return f"image2: the candidate list lacks {sorted(need - pq)[:4]} or holds {sorted(pq - every)[:4]}"
        bad = differ(order, got[0], got[1], w)
        if bad:
            return bad
    return None
