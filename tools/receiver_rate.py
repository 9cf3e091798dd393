"""Cost of the receiver step (include/hare_hip.h, "receivers"; kernel hare_receive_reflect, receive.hip): hare_receive_device against
hare_bounce_device (last cast only) on the same burst, device-resident, HIP events on the launch stream; K = 1 / 8 / 64 receivers,
B = 1 / 8 bands, 4 000 bins; receiver 0 is the direct-sound case (a 1 m sphere 2 m from the source: ~7 % of the rays cross it in cast 0,
into one or two bins), timed with the wave-aggregated atomics and with the naive ones.  With --host, also the host alternative a caller
has without the feature: Bounce_batch(all_casts=True) and the numpy restatement of the step (tests/receive_ref.py) on every cast.
With --scatter SIGMA (K = 8, B = 8 only), the same loop again with a scattering table of SIGMA on every polygon and band (hare_receive_scatter
in place of hare_receive_reflect; SIGMA 0 runs that kernel on exactly the rays the specular loop has); run it under rocprofv3 --kernel-trace
for the two kernels' per-cast times.
With --rain (B = 8, K = 1 and 8; SIGMA from --scatter, default 0.3), the scattering loop with and without diffuse rain
(HARE_RECEIVE_DIFFUSE_RAIN), and a noise figure: the relative spread, over 8 scatter seeds, of the energy the receivers get from 60 m of
path on (summed over receivers and bands), with rain and without.
With --directional (B = 8; K = 8 and 64, or K = 1 and 8 with --rain; combinable with --scatter and --rain), every loop of the run is timed
again with HARE_RECEIVE_DIRECTIONAL in the same run (the _dir kernels, a four-fold histogram): dir_ms, scatter_dir_ms, rain_dir_ms and
their cost over the same loop without the flag.  With --order 2,3 beside it, the specular loop again at those ambisonic orders
(HARE_RECEIVE_ORDER2 / _ORDER3: the _dir2 / _dir3 kernels, nine and sixteen channels): dir2_ms, dir3_ms, the highest order with
"receive_aggregate" 0 too, and next to every dir row the spread of its timed runs, (max - min) / median in percent.
With --time-limit and / or --floor-bits N [--roulette] (the header's "Termination"), the specular loop of every (K, B) again with the time
limit, with the energy floor 2^-N, and with both where both are given: cut_*_ms against ms of the same row, and the share of the rays
still live -- over all casts (the loop's ray counter over n x bounces) and in the casts 1, 2, 4, 8, ... (the counter's difference between
two calls that differ by one cast).
With --source (K = 8, B = 8 only; nothing else of the above runs), the host wall time of hare_receive_source against hare_receive_batch
given the same rays (the source's own, downloaded once), without and with state_in: the three calls interleaved, the median of --reps
runs (default there: 9) after a warm-up, and the spread (min, max) of each; and hare_emit_source alone between HIP events, beside the
120 B per ray it writes at B = 8.  Run it under rocprofv3 --kernel-trace --stats for the kernel's own time.
With --map K[,K..] (B = 8, bins of 0.2 m: 1 000, or as many as the histogram cap leaves the largest K; nothing else of the above runs), the
receive loop with a receiver map (hare_scene_set_receiver_map; the _map kernels): the plain bounce loop, the linear loop at K = 256, the
map over the same 256 receivers, a plane of at most K receivers at 1.2 m for every K given, and a cloud of 4 096 in the room, interleaved,
the median of --reps runs; `over` is the time over the plain loop.  Run it under rocprofv3 --kernel-trace --stats for the kernels' times.
With --source --direct (B = 8, bins of 0.2 m; nothing else runs), the direct sound ("Direct sound": HARE_RECEIVE_DIRECT): the host wall time
of hare_receive_source with and without the flag, interleaved, the median of --reps runs and the spread of each, for K = 8 linear receivers
and for a plane of at most 4 096 receivers as a map; and the gain in noise -- the relative spread over 8 values of "source_seed" of one
mid-hall receiver's summed 0 - 50 ms window (band 0; 17.15 m of path), with and without the flag, beside the cast-0 rays that receiver got.
Run it under rocprofv3 --kernel-trace --stats for the three kernels' own times.
With --source --direct --image, the first-order image sources too ("Image sources (first order)": HARE_RECEIVE_IMAGE): the same run with two
more calls interleaved, `direct + image` with the pair search's pre-cull (scene option "image_cull" 1) and without it (0), their wall
times and the same noise figure for `direct + image`.  With --image-cull N as well (a profiling run: rocprofv3 --kernel-trace --stats, one
run per N, then tools/image_kernel_times.py on the two traces), only `direct` and `direct + image` with "image_cull" N run, and no noise.
With --source --direct --image --image2, the second-order image sources ("Image sources (second order)": HARE_RECEIVE_IMAGE2): per layout,
first a probe -- hare_image2_device alone on lists of 2^26 candidates and 2^24 paths, with "image2_prune" 1 and 0 (or only N with
--image2-prune N: a profiling run under rocprofv3 --kernel-trace --stats, condensed by tools/image_kernel_times.py), its candidate and path
counts and its device time (events around the call; median, min .. max) -- then, if the counts fit lists of 2^26, the options
"image2_max_cands" / "image2_max_paths" set to the next powers of two and `direct + image` against `direct + image + image2`, interleaved,
wall time and the same noise figure.
Prints ONE JSON line.  usage: python tools/receiver_rate.py [hall|cathedral] [--rays N] [--bounces B] [--reps R] [--host] [--quick]
                                                          [--scatter SIGMA] [--rain] [--directional [--order N[,N]]] [--time-limit] [--floor-bits N [--roulette]]
                                                          [--source [--direct [--image [--image-cull N] [--image2 [--image2-prune N]]]]] [--map K[,K..]]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import hare_amd as H

ap = argparse.ArgumentParser()
ap.add_argument("scene", nargs="?", default="hall", choices=["hall", "cathedral"])
ap.add_argument("--rays", type=int, default=1 << 20)
ap.add_argument("--bounces", type=int, default=8)
ap.add_argument("--reps", type=int, default=None, help="timed runs per figure (default 10; 9 with --source)")
ap.add_argument("--host", action="store_true", help="also time Bounce_batch(all_casts=True) + the numpy step (K = 8, B = 8)")
ap.add_argument("--quick", action="store_true", help="K = 8, B = 8 only (a profiling run)")
ap.add_argument("--scatter", type=float, default=None, metavar="SIGMA",
                help="K = 8, B = 8 only, and the loop again with a scattering table of SIGMA everywhere (scene option scatter_seed 1)")
ap.add_argument("--rain", action="store_true", help="K = 1 and 8, B = 8: the scattering loop with and without diffuse rain, and its noise")
ap.add_argument("--directional", action="store_true", help="B = 8: every loop again with HARE_RECEIVE_DIRECTIONAL, in the same run")
ap.add_argument("--order", default="", metavar="N[,N]", help="with --directional: the loop again at ambisonic order 2 and / or 3 (HARE_RECEIVE_ORDER2 / _ORDER3), "
                "each row with the spread of its timed runs; the highest order also with \"receive_aggregate\" 0")
ap.add_argument("--time-limit", action="store_true", help="the loop again with HARE_RECEIVE_TIME_LIMIT")
ap.add_argument("--floor-bits", type=int, default=0, metavar="N", help="the loop again with the energy floor 2^-N (scene option receive_floor_bits)")
ap.add_argument("--roulette", action="store_true", help="with --floor-bits: Russian roulette under the floor (scene option receive_roulette)")
ap.add_argument("--source", action="store_true", help="K = 8, B = 8: hare_receive_source against hare_receive_batch from host rays, wall time")
ap.add_argument("--direct", action="store_true", help="with --source: hare_receive_source with and without HARE_RECEIVE_DIRECT, time and noise")
ap.add_argument("--image", action="store_true", help="with --source --direct: also direct + HARE_RECEIVE_IMAGE, with and without the pair search's pre-cull")
ap.add_argument("--image-cull", type=int, default=None, choices=[0, 1], metavar="N", help="with --image: a profiling run with \"image_cull\" N only")
ap.add_argument("--image2", action="store_true", help="with --source --direct --image: also direct + image + HARE_RECEIVE_IMAGE2, its counts, times and noise")
ap.add_argument("--image2-prune", type=int, default=None, choices=[0, 1], metavar="N", help="with --image2: a profiling run, the probe with \"image2_prune\" N only")
ap.add_argument("--map", default=None, metavar="K[,K..]", help="B = 8: receiver maps (planes of about K receivers, a cloud of 4096) against the linear loop at K = 256")
a = ap.parse_args()
if a.reps is None:
    a.reps = 9 if a.source else 10
if a.rain and a.scatter is None:
    a.scatter = 0.3
if not torch.cuda.is_available():
    sys.exit("receiver_rate: no GPU -- nothing to measure")

D = 64 if a.scene == "hall" else 128
mesh = H.scenes.SCENES[a.scene]()
T = H.Topology(mesh.verts, mesh.nverts)
g = H.Voxel_Grid([T], D)
n, nb, N_BINS, BIN_LEN, FRAC = a.rays, a.bounces, 4000, 0.05, 32
rays = H.scenes.burst_rays(n, mesh.size)
st = torch.cuda.current_stream().cuda_stream
d_src = torch.from_numpy(rays).cuda()
d_rays = torch.empty_like(d_src)
d_work = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
d_last = torch.zeros(n * 56, dtype=torch.uint8, device="cuda")
S = np.array([0.31, 0.42, 0.37]) * np.asarray(mesh.size)


def receivers(K):
    rng = np.random.default_rng(K)
    c = [S + np.array([2.0, 0.0, 0.0])]                                 # the direct sound: r = 1 m at 2 m
    c += list(rng.uniform(0.1, 0.9, (K - 1, 3)) * np.asarray(mesh.size))
    return np.array(c), np.concatenate([[1.0], rng.uniform(0.3, 1.0, K - 1)])


def source_run():
    """hare_receive_source against hare_receive_batch on the same rays, host wall time (what a caller with host buffers sees)."""
    K, B = 8, 8
    c, r = receivers(K)
    g.set_receivers(c, r).set_absorption(np.random.default_rng(B).uniform(0.02, 0.3, (T.Polygon_Count, B)))
    g.set_source(S, power=np.ones(B)).set_option("source_seed", 1)
    d_r = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    d_s = torch.empty((1 + B, n), dtype=torch.float64, device="cuda")
    ms = []
    for _ in range(a.reps + 1):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        g.emit_device(n, d_r.data_ptr(), d_s.data_ptr(), stream=st)
        e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    emit_ms = float(np.median(ms[1:]))
    src_rays, src_state = d_r.cpu().numpy(), d_s.cpu().numpy()
    calls = {"source": lambda: g.Receive_source(n, nb, N_BINS, BIN_LEN, frac_bits=FRAC),
             "batch": lambda: g.Receive_batch(src_rays, nb, N_BINS, BIN_LEN, frac_bits=FRAC),
             "batch_state_in": lambda: g.Receive_batch(src_rays, nb, N_BINS, BIN_LEN, energy=src_state, frac_bits=FRAC)}
    res = {k: f() for k, f in calls.items()}                              # the warm-up; and the three compute the same
    same = all(res["source"][i].tobytes() == res["batch_state_in"][i].tobytes() for i in (0, 2, 3))
    wall = {k: [] for k in calls}
    for _ in range(a.reps):                                               # interleaved: drift of the host or the link meets all three alike
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    row = {"scene": a.scene, "domain": D, "rays": n, "bounces": nb, "K": K, "B": B, "reps": a.reps, "same_bytes": bool(same),
           "emit_ms": round(emit_ms, 4), "emit_bytes_per_ray": 48 + 8 * (1 + B), "emit_GBps": round(n * (48 + 8 * (1 + B)) / emit_ms / 1e6, 1),
           "emit_Mrays_s": round(n / emit_ms / 1e3, 1)}
    for k, v in wall.items():
        row[k + "_ms"] = round(float(np.median(v)), 3)
        row[k + "_min_max_ms"] = [round(min(v), 3), round(max(v), 3)]
    row["source_over_batch"] = round(row["source_ms"] / row["batch_ms"], 3)
    row["source_over_batch_state_in"] = round(row["source_ms"] / row["batch_state_in_ms"], 3)
    print(json.dumps(row))


def image2_probe(p, K, B, n_bins, bin_len, prunes):
    """hare_image2_device alone on lists nothing overflows but the unpruned hall: counts and device time per "image2_prune"."""
    C, M = 1 << 26, 1 << 24
    d_w = torch.empty(H.Voxel_Grid.image2_work_bytes(T.Polygon_Count, C, M), dtype=torch.uint8, device="cuda")
    d_h = torch.zeros(K * n_bins * B, dtype=torch.int64, device="cuda")
    d_d = torch.zeros(2 * K, dtype=torch.int64, device="cuda")
    out = {"max_cands": C, "max_paths": M}
    for prune in prunes:
        p.set_option("image2_prune", prune)
        ms = []
        for rep in range(4 if prune == 0 else a.reps + 1):              # the first is the warm-up
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            p.Image2_device(n, n_bins, bin_len, FRAC, C, M, d_w.data_ptr(), d_h.data_ptr(), d_d.data_ptr(), stream=st)
            e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
            print("image2 probe", K, "prune", prune, "rep", rep, round(ms[-1], 3), "ms", file=sys.stderr, flush=True)
        cnt = d_w[:16].cpu().numpy().view(np.uint64)
        out["prune%d" % prune] = {"cands": int(cnt[0]), "paths": int(cnt[1]) if int(cnt[0]) <= C else None, "fits": bool(cnt[0] <= C and cnt[1] <= M),
                                  "device_ms": round(float(np.median(ms[1:])), 3), "device_min_max_ms": [round(min(ms[1:]), 3), round(max(ms[1:]), 3)]}
    p.set_option("image2_prune", 1)
    return out


def direct_run():
    """hare_receive_source with and without HARE_RECEIVE_DIRECT: host wall time, and the spread of a mid-hall receiver's early energy."""
    B, bin_len, n_bins = 8, 0.2, 1000
    size = np.asarray(mesh.size)
    alpha = np.random.default_rng(B).uniform(0.02, 0.3, (T.Polygon_Count, B))
    spacing = float(np.sqrt(size[0] * size[1] / 4096))
    while (int(size[0] // spacing) + 1) * (int(size[1] // spacing) + 1) > 4096:
        spacing *= 1.002
    plane = H.Voxel_Grid.receiver_plane([0.0, 0.0], size[:2], 1.2, spacing, 0.25)
    layouts = {"linear_8": receivers(8) + (False,), "plane_4096": plane + (True,)}
    early = int(np.ceil(17.15 / bin_len))                                 # 50 ms of path at 343 m/s
    rows = {}
    for name, (c, r, as_map) in layouts.items():
        p = H.Voxel_Grid([T], D)
        (p.set_receiver_map if as_map else p.set_receivers)(c, r)
        p.set_absorption(alpha)
        p.set_source(S, power=np.ones(B)).set_option("source_seed", 1)
        calls = {"plain": lambda p=p: p.Receive_source(n, nb, n_bins, bin_len, frac_bits=FRAC),
                 "direct": lambda p=p: p.Receive_source(n, nb, n_bins, bin_len, frac_bits=FRAC, direct=True)}
        if a.image:
            def imaged(cull, p=p):
                p.set_option("image_cull", cull)
                return p.Receive_source(n, nb, n_bins, bin_len, frac_bits=FRAC, direct=True, image=True)
            if a.image_cull is None:
                calls["direct_image"] = lambda: imaged(1)
                calls["direct_image_nocull"] = lambda: imaged(0)
            else:
                del calls["plain"]
                calls["direct_image"] = lambda: imaged(a.image_cull)
        probe = None
        if a.image2:
            probe = image2_probe(p, int(c.shape[0]), B, n_bins, bin_len, (1, 0) if a.image2_prune is None else (a.image2_prune,))
            if a.image2_prune is not None:                                # a profiling run: counts and the profiler's kernel times
                rows[name] = {"K": int(c.shape[0]), "map": as_map, "image2_probe": probe}
                continue
            calls = {"direct_image": lambda: imaged(1)}
            best = probe["prune1"]
            if best["fits"]:
                p.set_option("image2_max_cands", max(1024, 1 << int(best["cands"] - 1).bit_length()))
                p.set_option("image2_max_paths", max(1024, 1 << int(best["paths"] - 1).bit_length()))
                calls["direct_image2"] = lambda p=p: p.Receive_source(n, nb, n_bins, bin_len, frac_bits=FRAC, direct=True, image=True, image2=True)
        for f in calls.values():
            f()                                                           # the warm-up
        wall = {k: [] for k in calls}
        for _ in range(a.reps):                                           # interleaved
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                wall[k].append((time.perf_counter() - t0) * 1e3)
        row = {"K": int(c.shape[0]), "map": as_map}
        if probe is not None:
            row["image2_probe"] = probe
            row["image2_lists"] = [p.get_option("image2_max_cands"), p.get_option("image2_max_paths")]
        for k, v in wall.items():
            row[k + "_ms"] = round(float(np.median(v)), 3)
            row[k + "_min_max_ms"] = [round(min(v), 3), round(max(v), 3)]
        if "plain" in calls:
            row["direct_over_plain"] = round(row["direct_ms"] / row["plain_ms"], 4)
        if "direct_image2" in calls:
            row["image2_added_ms"] = round(row["direct_image2_ms"] - row["direct_image_ms"], 3)
        if a.image and "direct" in calls:
            row["image_added_ms"] = round(row["direct_image_ms"] - row["direct_ms"], 3)
        if "direct_image_nocull" in calls:
            row["image_nocull_added_ms"] = round(row["direct_image_nocull_ms"] - row["direct_ms"], 3)
        if a.image_cull is not None:                                      # a profiling run: the kernels' times are the profiler's business
            row["image_cull"] = a.image_cull
            rows[name] = row
            continue
        # the noise: one receiver about the middle of the hall, seen from the source
        mid = int(np.argmin(((c - size * np.array([0.6, 0.5, 0.0]) - np.array([0, 0, c[0, 2]])) ** 2).sum(axis=1))) if as_map else 0
        e = {k: [] for k in calls if k != "direct_image_nocull"}
        cast0 = []
        for seed in range(8):
            p.set_option("source_seed", 100 + seed)
            for k, f in calls.items():
                if k not in e:
                    continue
                e[k].append(float(f()[0][mid, :early, 0].astype(np.float64).sum()) * 2.0 ** -FRAC)
            cast0.append(int(p.Receive_source(n, 1, n_bins, bin_len, frac_bits=FRAC)[2][mid].sum()))
        row["receiver"] = mid
        row["receiver_distance_m"] = round(float(np.linalg.norm(c[mid] - S)), 3)
        row["receiver_radius_m"] = round(float(r[mid]), 3)
        row["cast0_rays"] = cast0
        for k in e:
            row["early_spread_" + k] = round(float(np.std(e[k], ddof=1) / np.mean(e[k])), 6)
            row["early_mean_" + k] = round(float(np.mean(e[k])), 4)
        rows[name] = row
        print(json.dumps({name: row}), file=sys.stderr, flush=True)
    print(json.dumps({"scene": a.scene, "domain": D, "rays": n, "bounces": nb, "B": B, "n_bins": n_bins, "bin_len": bin_len, "reps": a.reps,
                      "early_bins": early, "rows": rows}))


if a.source:
    direct_run() if a.direct else source_run()
    sys.exit(0)


def bounce():
    g.bounce_device(n, d_rays.data_ptr(), nb, d_work.data_ptr(), d_events_last=d_last.data_ptr(), stream=st)


def map_run():
    """The receive loop with a map against the plain bounce loop and the linear loop at K = 256, every loop on a scene of its own."""
    B, bin_len = 8, 0.2
    size = np.asarray(mesh.size)
    alpha = np.random.default_rng(B).uniform(0.02, 0.3, (T.Polygon_Count, B))
    c256, r256 = receivers(256)
    r256 = np.minimum(r256, 0.3)                                          # map-sized spheres (the linear rows above use up to 1 m)
    layouts = {"linear_256": (c256, r256, False), "map_256": (c256, r256, True)}
    for K in [int(x) for x in a.map.split(",")]:
        spacing = float(np.sqrt(size[0] * size[1] / K))
        while (int(size[0] // spacing) + 1) * (int(size[1] // spacing) + 1) > K:      # the lattice's border rows: at most K receivers
            spacing *= 1.002
        c, r = H.Voxel_Grid.receiver_plane([0.0, 0.0], size[:2], 1.2, spacing, min(0.4 * spacing, 0.3))
        assert c.shape[0] <= K
        layouts["plane_%d" % K] = (c, r, True)
    rng = np.random.default_rng(4096)
    layouts["cloud_4096"] = (rng.uniform(0.05, 0.95, (4096, 3)) * size, np.full(4096, 0.3), True)
    n_bins = min(1000, (1 << 27) // (max(v[0].shape[0] for v in layouts.values()) * B))      # the histogram cap, from the K laid out
    init = torch.cat([torch.zeros((1, n), dtype=torch.float64, device="cuda"), torch.ones((B, n), dtype=torch.float64, device="cuda")])
    d_state = torch.empty_like(init)
    runs = {"bounce": bounce}
    rows = {"bounce": {}}
    keep = []
    for name, (c, r, as_map) in layouts.items():
        p = H.Voxel_Grid([T], D)
        (p.set_receiver_map if as_map else p.set_receivers)(c, r)
        p.set_absorption(alpha)
        K = c.shape[0]
        d_hist = torch.zeros(K * n_bins * B, dtype=torch.int64, device="cuda")
        d_det = torch.zeros(2 * K, dtype=torch.int64, device="cuda")
        keep.append((p, d_hist, d_det))
        runs[name] = (lambda p=p, d_hist=d_hist, d_det=d_det: p.receive_device(n, d_rays.data_ptr(), nb, n_bins, bin_len, FRAC, d_state.data_ptr(),
                                                                               d_work.data_ptr(), d_last.data_ptr(), d_hist.data_ptr(),
                                                                               d_det.data_ptr(), stream=st))
        rows[name] = {"K": K, "cells": p.get_option("receiver_map_cells")}
    ms = {k: [] for k in runs}
    for rep in range(a.reps + 1):                                         # interleaved; the first round warms up
        for name, fn in runs.items():
            d_rays.copy_(d_src); d_state.copy_(init)
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record(); torch.cuda.synchronize()
            if rep:
                ms[name].append(e0.elapsed_time(e1))
    base = float(np.median(ms["bounce"]))
    for (name, row), kept in zip(list(rows.items())[1:], keep):
        det = kept[2].cpu().numpy().reshape(-1, 2)
        row["detections_per_call"] = int(det.sum()) // (a.reps + 1)
        row["receivers_hit"] = int((det.sum(axis=1) > 0).sum())
    for name, row in rows.items():
        row["ms"] = round(float(np.median(ms[name])), 3)
        row["min_max_ms"] = [round(min(ms[name]), 3), round(max(ms[name]), 3)]
        row["over"] = round(row["ms"] / base, 3)
    same = keep[0][1].cpu().numpy().tobytes() == keep[1][1].cpu().numpy().tobytes()
    print(json.dumps({"scene": a.scene, "domain": D, "rays": n, "bounces": nb, "B": B, "n_bins": n_bins, "bin_len": bin_len, "reps": a.reps,
                      "map_256_same_bytes_as_linear_256": bool(same), "rows": rows}))


if a.map:
    map_run()
    sys.exit(0)


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        d_rays.copy_(d_src)                                              # both loops overwrite their rays: the copy is outside the window
        e0.record()
        fn()
        e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    global last_spread_pct
    last_spread_pct = round(100.0 * (max(ms) - min(ms)) / float(np.median(ms)), 2)      # of the call just timed: (max - min) / median
    return float(np.median(ms))


ms_bounce = timed(bounce, a.reps)
out = {"scene": a.scene, "domain": D, "rays": n, "bounces": nb, "n_bins": N_BINS, "bounce_ms": round(ms_bounce, 3),
       "bounce_Mcasts_s": round(n * nb / ms_bounce / 1e3, 1), "receive": []}
cases = [(1, 8), (8, 8)] if a.rain else ([(8, 8)] if a.quick else [(8, 8), (64, 8)]) if a.directional else ([(8, 8)] if (a.quick or a.scatter is not None) else [(K, B) for K in (1, 8, 64) for B in (1, 8)])
d_work_rain = torch.zeros(H.Voxel_Grid.receive_work_bytes(n, rain=True), dtype=torch.uint8, device="cuda") if a.rain else None
for K, B in cases:
    c, r = receivers(K)
    g.set_receivers(c, r)
    g.set_absorption(np.random.default_rng(B).uniform(0.02, 0.3, (T.Polygon_Count, B)))
    d_state = torch.empty((1 + B, n), dtype=torch.float64, device="cuda")
    init = torch.cat([torch.zeros((1, n), dtype=torch.float64, device="cuda"), torch.ones((B, n), dtype=torch.float64, device="cuda")])
    d_hist = torch.zeros(K * N_BINS * B, dtype=torch.int64, device="cuda")
    d_det = torch.zeros(2 * K, dtype=torch.int64, device="cuda")
    orders = [int(x) for x in a.order.split(",") if x] if a.directional else []
    d_hist4 = torch.zeros(K * N_BINS * B * H.capi.ORDER_CHANNELS[max(orders + [1])], dtype=torch.int64, device="cuda") if a.directional else None

    def receive(rain=False, directional=False, time_limit=False, casts=nb, d_counters=0, order=1):
        g.receive_device(n, d_rays.data_ptr(), casts, N_BINS, BIN_LEN, FRAC, d_state.data_ptr(), (d_work_rain if rain else d_work).data_ptr(),
                         d_last.data_ptr(), (d_hist4 if directional else d_hist).data_ptr(), d_det.data_ptr(), stream=st, rain=rain,
                         directional=directional, time_limit=time_limit, d_counters=d_counters, **({"order": order} if order > 1 else {}))

    def timed_cut(row, key, time_limit, floor_bits):                     # the specular loop under a rule, against row["ms"]
        g.set_option("receive_floor_bits", floor_bits).set_option("receive_roulette", int(a.roulette and floor_bits > 0))
        ms = timed(lambda: (d_state.copy_(init), receive(time_limit=time_limit)), a.reps)
        row[key + "_ms"] = round(ms - ms_copy, 3)
        row[key + "_of_plain"] = round((ms - ms_copy) / row["ms"], 3)
        d_ctr = torch.zeros(8, dtype=torch.int64, device="cuda")

        def cast_rays(casts):                                            # rays cast by a call of `casts` casts, over all of them
            d_ctr.zero_(); d_rays.copy_(d_src); d_state.copy_(init)
            receive(time_limit=time_limit, casts=casts, d_counters=d_ctr.data_ptr()); torch.cuda.synchronize()
            return int(d_ctr[0].item())
        row[key + "_live_share"] = round(cast_rays(nb) / (n * nb), 4)
        at = [c for c in (1, 2, 4, 8, 16, 32, 64, 128, 255) if c < nb]
        row[key + "_live_in_cast"] = {c: round((cast_rays(c + 1) - cast_rays(c)) / n, 4) for c in at}
        g.set_option("receive_floor_bits", 0).set_option("receive_roulette", 0)

    def timed_dir(row, key, base_key, rain=False, order=1):              # the same loop with the flag, against row[base_key]
        ms = timed(lambda: (d_state.copy_(init), receive(rain, True, order=order)), a.reps)
        row[key] = round(ms - ms_copy, 3)
        row[key.replace("ms", "spread_pct")] = last_spread_pct
        row[key.replace("ms", "over_pct")] = round(100.0 * (ms - ms_copy - row[base_key]) / row[base_key], 1)
        row[key.replace("ms", "over_bounce_pct")] = round(100.0 * (ms - ms_copy - ms_bounce) / ms_bounce, 1)
    row = {"K": K, "B": B}
    for agg in ((1, 0) if K == 8 and B == 8 and a.scatter is None and not a.rain and not a.directional else (1,)):
        g.set_option("receive_aggregate", agg)
        d_hist.zero_(); d_det.zero_()
        d_state.copy_(init)
        ms = timed(lambda: (d_state.copy_(init), receive()), a.reps)
        ms_copy = timed(lambda: d_state.copy_(init), a.reps)          # the state reset inside the window, timed alone
        key = "ms" if agg else "ms_naive"
        row[key] = round(ms - ms_copy, 3)
        row[key.replace("ms", "over_bounce_pct")] = round(100.0 * (ms - ms_copy - ms_bounce) / ms_bounce, 1)
    g.set_option("receive_aggregate", 1)
    if a.directional:
        timed_dir(row, "dir_ms", "ms")
        g.set_option("receive_aggregate", 0)
        timed_dir(row, "dir_naive_ms", "ms")
        g.set_option("receive_aggregate", 1)
        for order in orders:
            timed_dir(row, "dir%d_ms" % order, "ms", order=order)
        if orders:
            g.set_option("receive_aggregate", 0)
            timed_dir(row, "dir%d_naive_ms" % max(orders), "ms", order=max(orders))
            g.set_option("receive_aggregate", 1)
    if a.time_limit:
        timed_cut(row, "cut_time", True, 0)
    if a.floor_bits:
        timed_cut(row, "cut_floor", False, a.floor_bits)
    if a.time_limit and a.floor_bits:
        timed_cut(row, "cut_both", True, a.floor_bits)
    d_hist.zero_(); d_det.zero_(); d_rays.copy_(d_src); d_state.copy_(init)
    receive(); torch.cuda.synchronize()
    det = d_det.cpu().numpy().reshape(K, 2)
    row["direct_frac_cast_sum"] = round(float(det[0].sum()) / n, 4)     # detections of receiver 0 (all casts) per ray
    row["detections"] = int(det.sum())
    if a.scatter is not None:                                            # the same loop with diffuse scattering
        g.set_scattering(np.full((T.Polygon_Count, B), a.scatter)).set_option("scatter_seed", 1)
        ms = timed(lambda: (d_state.copy_(init), receive()), a.reps)
        row["scatter_sigma"] = a.scatter
        row["scatter_ms"] = round(ms - ms_copy, 3)
        row["scatter_over_specular_pct"] = round(100.0 * (ms - ms_copy - row["ms"]) / row["ms"], 1)
        if a.directional:
            timed_dir(row, "scatter_dir_ms", "scatter_ms")
        d_hist.zero_(); d_det.zero_(); d_rays.copy_(d_src); d_state.copy_(init)
        receive(); torch.cuda.synchronize()
        row["scatter_detections"] = int(d_det.cpu().numpy().sum())
        if a.rain:                                                       # the same loop with diffuse rain
            ms = timed(lambda: (d_state.copy_(init), receive(True)), a.reps)
            row["rain_ms"] = round(ms - ms_copy, 3)
            row["rain_over_scatter"] = round((ms - ms_copy) / row["scatter_ms"], 2)
            if a.directional:
                timed_dir(row, "rain_dir_ms", "rain_ms", rain=True)
            late = int(60.0 / BIN_LEN)
            for rain in (False, True):
                e = []
                for seed in range(8):
                    g.set_option("scatter_seed", 100 + seed)
                    d_hist.zero_(); d_det.zero_(); d_rays.copy_(d_src); d_state.copy_(init)
                    receive(rain); torch.cuda.synchronize()
                    h = d_hist.cpu().numpy().view(np.uint64).reshape(K, N_BINS, B)
                    e.append(float(h[:, late:, :].astype(np.float64).sum()) * 2.0 ** -FRAC)
                row["late_spread_rain" if rain else "late_spread"] = round(float(np.std(e, ddof=1) / np.mean(e)), 5)
            g.set_option("scatter_seed", 1)
        g.set_scattering(None)
    out["receive"].append(row)
    print(json.dumps(row), file=sys.stderr, flush=True)

if a.host:
    from tests.receive_ref import replay_loop
    from oracle import pyoracle as po
    K, B = 8, 8
    c, r = receivers(K)
    alpha = np.random.default_rng(B).uniform(0.02, 0.3, (T.Polygon_Count, B))
    t0 = time.perf_counter()
    ev, _ = g.Bounce_batch(rays, nb, all_casts=True)
    t1 = time.perf_counter()
    To = po.Topology(mesh.verts, mesh.nverts)
    replay_loop(po, To, rays, ev, c, r, N_BINS, BIN_LEN, FRAC, alpha=alpha)
    t2 = time.perf_counter()
    out["host_alternative"] = {"K": K, "B": B, "bounce_all_casts_ms": round((t1 - t0) * 1e3, 1), "numpy_step_ms": round((t2 - t1) * 1e3, 1),
                               "events_bytes": int(ev.nbytes)}
print(json.dumps(out))
