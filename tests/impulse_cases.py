"""The cases of the tests of the impulses (tests/test_impulse_cases.py on the reference alone, tests/test_gpu_impulses.py on the device): a
case type, a fixed list that reaches each edge of the definition and of the kernel's plan at the smallest shape that has it, a seeded
sweep of 50, inputs from a seed, and the reference (tests/impulse_ref.py) computed once per case.  The kernel's tile and chunk are read
from hare_amd/csrc/hare_device.h.  No GPU, no torch."""
import os
import re
from functools import lru_cache

import numpy as np

from tests.impulse_ref import impulse_ref

_DEVICE_H = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hare_amd", "csrc", "hare_device.h")).read()
THREADS = int(re.search(r"constexpr int kImpulseThreads = (\d+);", _DEVICE_H).group(1))
assert re.search(r"constexpr int kImpulseTile = kImpulseThreads;", _DEVICE_H) and re.search(r"constexpr int kImpulseChunk = kImpulseThreads;", _DEVICE_H)
TILE = CHUNK = THREADS

SENTINEL = 0x7FF8DEADBEEF0000          # what `out` holds before a call with add == 0: a NaN pattern no sum produces
INT64_MIN = -(1 << 63)
SEED = 9100


def plan(K, B, C, T, n_out):
    """impulses_plan's launch: (grid, block, dynamic LDS bytes)"""
    return K * -(-n_out // TILE), THREADS, 8 * B * T + CHUNK * (8 * (C + 2) + 4) + 4 * (THREADS // 64)


class Case:
    """entries: "none"; "dense" (every bin and band); a float (the chance of an entry per bin and band); or a tuple of (bin, band) pairs,
    a negative bin counted from the end, the same for every receiver.  words: "normal" (W in [1, 2^40), channel words within +-W);
    "edge" (the W words 1, 2^53 + 1 and 2^64 - 1 going round, channel words among them negative ones and INT64_MIN).  weight: None;
    "plain" (random uint32); "empties" (0 at the first entry, whose hW stays non-zero, 1 at the second: floor(h / 2^32)).  taps: "normal";
    "negative"; "denormal"; "huge" (2^+-500); "inf" / "nan" (ONE such tap among normals: the device call only).  window: "whole", "one",
    "head", "tail", "tile" (across the first tile edge of the whole call).  gap: out_stride - n_out.  add: None, or what the rows hold
    before: "normal", "zeros" (-0.0 among +0.0) or "nan" (one NaN per row among normals)."""

    def __init__(self, index, name, K, n_bins, B, C, T, entries, words="normal", weight=None, taps="normal", frac_bits=24, window="whole", gap=0, add=None):
        self.index, self.name, self.K, self.n_bins, self.B, self.C, self.T = index, name, K, n_bins, B, C, T
        self.entries, self.words, self.weight, self.taps, self.frac_bits, self.window, self.gap, self.add = entries, words, weight, taps, frac_bits, window, gap, add
        total = n_bins + T - 1
        self.n0, self.n_out = {"whole": (0, total), "one": (total // 2, 1), "head": (0, max(1, min(T - 1, n_bins))),
                               "tail": (max(T - 1, n_bins - 1), total - max(T - 1, n_bins - 1)), "tile": (TILE - 2, 4)}[window]
        assert self.n0 >= 0 and self.n_out >= 1 and self.n0 + self.n_out <= total, name
        self.stride = self.n_out + gap
        self.device_only = taps in ("inf", "nan")
        self.id = f"{index}-{name}-K{K}-n{n_bins}-B{B}-C{C}-T{T}"

    def positions(self):
        return [(i % self.n_bins if i < 0 else i, b) for i, b in self.entries] if isinstance(self.entries, tuple) else None


@lru_cache(maxsize=None)
def inputs(case):
    """dict(hist uint64 [K, n_bins, B, C], taps float64 [B, T], weight uint32 [n_bins, B] or None, out0 float64 [K, C, stride]), read-only"""
    rng = np.random.default_rng(SEED + case.index)
    K, nb, B, C, T = case.K, case.n_bins, case.B, case.C, case.T
    there = np.zeros((K, nb, B), bool)
    if case.entries == "dense":
        there[...] = True
    elif isinstance(case.entries, float):
        there = rng.random((K, nb, B)) < case.entries
    elif case.entries != "none":
        for i, b in case.positions():
            there[:, i, b] = True
    if case.words == "edge":
        W = np.array([1, (1 << 53) + 1, (1 << 64) - 1], np.uint64)[np.arange(K * nb * B).reshape(K, nb, B) % 3]
    else:
        W = rng.integers(1, 1 << 40, (K, nb, B), dtype=np.uint64)
    W = np.where(there, W, np.uint64(0))
    hist = np.zeros((K, nb, B, C), np.uint64)
    hist[..., 0] = W
    if C > 1:
        if case.words == "edge":
            pool = np.array([-1, 1, INT64_MIN, -(1 << 53) - 1, (1 << 62) + 1, 0, -3], np.int64)
            sub = pool[rng.integers(0, len(pool), (K, nb, B, C - 1))]
        else:
            sub = np.trunc(rng.uniform(-1, 1, (K, nb, B, C - 1)) * W[..., None].astype(np.float64)).astype(np.int64)
        hist[..., 1:] = np.where(there[..., None], sub, 0).view(np.uint64)
    weight = None
    if case.weight == "plain":
        weight = rng.integers(0, 1 << 32, (nb, B), dtype=np.uint32)
    elif case.weight == "empties":
        weight = rng.integers(1 << 31, 1 << 32, (nb, B), dtype=np.uint32)
        (i0, b0), (i1, b1) = case.positions()[:2]
        weight[i0, b0], weight[i1, b1] = 0, 1
    taps = rng.standard_normal((B, T))
    if case.taps == "negative":
        taps = -np.abs(taps)
    elif case.taps == "denormal":
        taps = rng.integers(1, 1 << 50, (B, T)).astype(np.float64) * 5e-324 * rng.choice([-1.0, 1.0], (B, T))
    elif case.taps == "huge":
        taps = np.ldexp(rng.uniform(1.0, 2.0, (B, T)), rng.choice([-500, 500], (B, T))) * rng.choice([-1.0, 1.0], (B, T))
    elif case.taps in ("inf", "nan"):
        taps[B // 2, T // 3] = np.inf if case.taps == "inf" else np.nan
    if case.add is None:
        out0 = np.full((K, C, case.stride), SENTINEL, np.uint64).view(np.float64)
    else:
        out0 = rng.standard_normal((K, C, case.stride))
        if case.add == "zeros":
            out0[...] = np.where(rng.random(out0.shape) < 0.5, -0.0, 0.0)
        elif case.add == "nan":
            out0[..., 0] = np.nan
    r = dict(hist=hist, taps=np.ascontiguousarray(taps), weight=weight, out0=out0)
    for a in r.values():
        if a is not None:
            a.flags.writeable = False
    return r


@lru_cache(maxsize=None)
def reference(case):
    """float64 [K, C, stride]: out0 with the window written or added onto"""
    x = inputs(case)
    y = impulse_ref(x["hist"], x["taps"], case.frac_bits, case.n0, case.n_out, x["weight"], out=x["out0"], add=0 if case.add is None else 1)
    y.flags.writeable = False
    return y


def entry_count(case):
    from tests.impulse_ref import entries
    x = inputs(case)
    return int((entries(x["hist"], x["weight"]) != 0).sum())


def _fixed():
    c = []

    def add(name, K, n_bins, B, C, T, entries, **kw):
        c.append(Case(len(c), name, K, n_bins, B, C, T, entries, **kw))

    # shapes: every T with n_bins around a wave, a chunk and a tile; channels, bands and receivers go round
    T_LIST, NB_LIST, C_LIST, B_LIST, K_LIST = [1, 2, 33, 1024], [1, 63, 64, 65, 255, 256, 257, 1025], [1, 4, 9, 16], [1, 3, 8], [1, 3]
    for j, nb in enumerate(NB_LIST):
        for i, T in enumerate(T_LIST):
            add("shape", K_LIST[(i + j) % 2], nb, B_LIST[(i + j) % 3], C_LIST[(i + j // 2) % 4], T, 0.1 if nb > 1 else "dense")
    add("receivers", 257, 5, 3, 4, 2, 0.5)
    add("none", 3, 300, 3, 4, 33, "none")
    # one entry: bin 0, the last bin, each side of a chunk edge (the scan of tile 0 starts at bin 0) and of a tile edge
    for name, at in (("first", 0), ("last", -1), ("chunk-", CHUNK - 1), ("chunk+", CHUNK), ("tile-", TILE - 1), ("tile+", TILE)):
        add("one-" + name, 1, 600, 3, 4, 33, ((at, 1),))
    add("one-chunk-of-tile-1", 1, 1200, 1, 1, 33, ((TILE - 32 + CHUNK - 1, 0), (TILE - 32 + CHUNK, 0)))      # tile 1 scans from TILE - 32: its chunk edge
    # two entries within T of each other in one band, and in two bands: the order of the sum
    add("two-one-band", 1, 100, 3, 4, 33, ((40, 1), (50, 1)))
    add("two-bands", 1, 100, 3, 4, 33, ((40, 2), (50, 0)))
    add("two-same-bin", 2, 100, 8, 9, 33, ((40, 0), (40, 7), (41, 3)))
    # (two terms commute: a third entry is what lets a wrong order show in the bits)
    add("three-one-band", 2, 100, 3, 9, 33, ((40, 1), (45, 1), (50, 1)))
    add("three-two-bands", 2, 100, 3, 9, 33, ((45, 0), (40, 2), (50, 2)))
    add("dense", 2, 300, 3, 4, 33, "dense")
    add("dense-16", 1, 300, 8, 16, 65, "dense")
    add("weight-plain", 2, 257, 3, 4, 33, 0.2, weight="plain")
    add("weight-empties", 1, 100, 3, 4, 33, ((40, 1), (45, 1), (50, 2)), weight="empties")
    add("words-edge", 2, 65, 3, 4, 33, 0.3, words="edge")
    add("words-edge-16", 1, 65, 1, 16, 2, "dense", words="edge")
    add("frac-0", 1, 65, 3, 4, 33, 0.3, frac_bits=0)
    add("frac-62", 1, 65, 3, 4, 33, 0.3, frac_bits=62, words="edge")
    for taps in ("negative", "denormal", "huge", "inf", "nan"):
        add("taps-" + taps, 2, 300, 3, 4, 33, 0.1, taps=taps)
    for window in ("one", "head", "tail", "tile"):
        add("window-" + window, 2, 600, 3, 4, 33, 0.1, window=window)
    add("window-tile-long", 1, 600, 3, 9, 1024, 0.1, window="tile")
    add("window-one-T1", 1, 600, 3, 1, 1, "dense", window="one")
    add("stride", 2, 300, 3, 4, 33, 0.1, gap=7)
    add("stride-window", 3, 300, 3, 16, 33, 0.1, gap=1, window="tail")
    for what in ("normal", "zeros", "nan"):
        add("add-" + what, 2, 300, 3, 4, 33, 0.1, add=what, gap=3 if what == "normal" else 0)
    return c


def _sweep(first):
    rng = np.random.default_rng(SEED)
    c = []
    for s in range(50):
        T = int(rng.choice([1, 2, 3, 17, 64, 65, 200, 511]))
        nb = int(rng.integers(1, 700))
        C, B, K = int(rng.choice([1, 4, 9, 16])), int(rng.integers(1, 9)), int(rng.integers(1, 4))
        c.append(Case(first + s, "sweep", K, nb, B, C, T, float(rng.choice([0.01, 0.05, 0.3, 1.0])), words=str(rng.choice(["normal", "edge"])),
                      weight=[None, "plain"][int(rng.integers(0, 2))], taps=str(rng.choice(["normal", "negative", "huge"])),
                      frac_bits=int(rng.integers(0, 63)), window=str(rng.choice(["whole", "one", "head", "tail"])), gap=int(rng.integers(0, 3)),
                      add=[None, None, "normal"][int(rng.integers(0, 3))]))
    return c


FIXED = _fixed()
SWEEP = _sweep(len(FIXED))
CASES = FIXED + SWEEP
