"""The cases of the device tests of the reduction (tests/test_gpu_hist_reduce.py): shapes at the kernel's tile, wave and carry edges in a
pairwise cover, with the word classes, windows, levels and weights dealt over them; inputs from a seed, and the reference
(tests/reduce_ref.py) computed once per case.  No GPU, no torch."""
from functools import lru_cache

import numpy as np

import hare_amd as H
from tests.reduce_ref import reduce_ref

N_BINS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097)
BANDS = (3, 5, 1, 8)            # in this order the largest shapes of the cover below stay small enough for the Python reference
RECEIVERS = (1, 3, 257)
CHANNELS = (1, 4)
WORDS = ("zero", "ones", "first", "last", "full", "small", "decay")
WEIGHTS = ("none", "zero", "ones", "random")
MAX32 = (1 << 32) - 1
DB31 = H.decay_levels(-np.arange(5.0, 36.0)).tolist()                      # the 31 levels -5 .. -35 dB


def shapes():
    """Every pair of values of two of (n_bins, B, K, channels) occurs: n_bins x B in full, K and channels dealt by the sum of the two
    indices (for a fixed n_bins or B the sum takes four or ten consecutive values: every residue mod 3 and mod 2; over all, every residue
    mod 6: every (K, channels))."""
    return [(n, B, RECEIVERS[(a + b) % 3], CHANNELS[(a + b) % 2]) for a, n in enumerate(N_BINS) for b, B in enumerate(BANDS)]


def windows(kind, n):
    if kind == 0:
        return []                                                           # levels only
    if kind == 1:
        return [(0, 0), (0, n), (n // 2, n // 2 + 1), (n, n), (n - 1, n), (0, 1)]          # empty, full, single bins
    if kind == 2:                                                           # edges on multiples of 64 and 256, plus or minus 1
        edges = [min(e, n) for e in (63, 64, 65, 255, 256, 257)]
        return [(0, e) for e in edges] + [(e, n) for e in edges] + [(edges[0], edges[3]), (edges[1], edges[4]), (edges[2], edges[5])]
    return [(j * n // 40, n - j * n // 50) for j in range(16)]               # 16 overlapping windows


def levels(kind):
    return [[], [0, 1, MAX32], DB31, [0, 1, MAX32] + DB31[:29]][kind]


def words(kind, shape, rng):
    K, n, B = shape[:3]
    if kind == "zero":
        return np.zeros(shape, np.uint64)
    if kind == "ones":
        return np.full(shape, (1 << 64) - 1, np.uint64)                    # carries into every hi word
    if kind in ("first", "last"):
        h = np.zeros(shape, np.uint64)
        h[rng.integers(K), 0 if kind == "first" else n - 1, rng.integers(B)] = rng.integers(1, 1 << 63, dtype=np.uint64)
        return h
    if kind == "full":
        return rng.integers(0, 1 << 64, shape, dtype=np.uint64)
    if kind == "small":
        return rng.integers(0, 1000, shape, dtype=np.uint64) * (rng.integers(0, 4, shape, dtype=np.uint64) == 0)
    i = np.arange(n, dtype=np.float64).reshape((1, n, 1) + (1,) * (len(shape) - 3))
    h = np.floor(2.0 ** 40 * 10.0 ** (-6.0 * i / n) * rng.uniform(0.5, 1.5, shape)).astype(np.uint64)       # an exponential decay
    return h


class Case:
    def __init__(self, index, n_bins, B, K, channels, word=None, win=None, lev=None, weight=None):
        self.n_bins, self.B, self.K, self.channels = n_bins, B, K, channels
        self.word = WORDS[index % 7] if word is None else word
        w, l = (index // 2) % 4 if win is None else win, (index // 3) % 4 if lev is None else lev
        if w == 0 and l == 0:
            l = 2
        self.win_kind, self.lev_kind = w, l
        self.weight_kind = WEIGHTS[(index // 5) % 4] if weight is None else weight
        self.index = index
        self.id = f"{index}-n{n_bins}-B{B}-K{K}-c{channels}-{self.word}-w{w}-l{l}-{self.weight_kind}"

    @property
    def windows(self):
        return windows(self.win_kind, self.n_bins)

    @property
    def levels(self):
        return levels(self.lev_kind)


@lru_cache(maxsize=None)
def inputs(case):
    """(hist [K, n_bins, B(, C)] uint64 with C = 4, 9 or 16, weight [n_bins, B] uint32 or None), from the case's seed."""
    rng = np.random.default_rng(1000 + case.index)
    shape = (case.K, case.n_bins, case.B) + ((case.channels,) if case.channels > 1 else ())
    hist = words(case.word, shape, rng)
    if case.channels > 1:
        hist[..., 1:] = rng.integers(0, 1 << 64, hist[..., 1:].shape, dtype=np.uint64)      # the channels 1 .. C - 1: never read
    wk = case.weight_kind
    weight = None if wk == "none" else (np.zeros((case.n_bins, case.B), np.uint32) if wk == "zero" else
                                        np.full((case.n_bins, case.B), MAX32, np.uint32) if wk == "ones" else
                                        rng.integers(0, 1 << 32, (case.n_bins, case.B), dtype=np.uint64).astype(np.uint32))
    return hist, weight


@lru_cache(maxsize=None)
def reference(case):
    hist, weight = inputs(case)
    return reduce_ref(hist, case.windows, case.levels, weight)


COVER = [Case(i, *s) for i, s in enumerate(shapes())]
# every word class with every weight at one shape that has idle threads (B = 3), a partial last tile and several tiles
CLASSES = [Case(100 + 4 * a + b, 300, 3, 3, 1 + 3 * (a % 2), word=w, win=3 if (a + b) % 2 else 2, lev=3, weight=x)
           for a, w in enumerate(WORDS) for b, x in enumerate(WEIGHTS)]
# the strides 9 and 16 of the higher orders' histograms (channel 0 of a word block of C): n_bins below a tile, one past 256 and several
# tiles; B with idle threads and full; words that differ from bin to bin, so that a read at another stride gives other sums
STRIDES = [Case(200 + 6 * a + 2 * b + c, n, (3, 8)[(a + b + c) % 2], 3, C, word=("full", "decay")[(b + c) % 2], win=2, lev=3, weight=("none", "random")[c])
           for a, C in enumerate((9, 16)) for b, n in enumerate((63, 257, 1000)) for c in range(2)]
