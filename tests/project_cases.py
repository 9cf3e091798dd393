"""The cases of the device tests of the projection (tests/test_gpu_hist_project.py): shapes at the kernel's tile, wave, sweep and carry
edges in a pairwise cover, with the word, coefficient and weight classes dealt over them; fixed cases that hold every class with every
weight, the higher channel counts and the vector counts around the kernel's sweep group; sweep_case(seed) for a seeded sweep; inputs from
a seed, and the reference (tests/project_ref.py) computed once per case.  A case holds at most MAX_ENTRIES = 2^20 histogram entries
(K x n_bins x B) and, beyond that, at most MAX_WORK = 2^23 entries x vectors (K x n_bins x B x J), so that the reference stays well under a
second; the only pair of values the two limits exclude from the cover is n_bins 4 097 with K 257.  No GPU, no torch.  tests/test_project_cases.py proves that the
cases hold what they name."""
from functools import lru_cache
from itertools import combinations

import numpy as np

from tests.project_ref import project_ref

GROUP = 8                        # vectors a sweep of the kernel carries (hare_amd/csrc/hare_device.h: kProjectGroup)
BANDS = (1, 3, 5, 8)
# the issue's sizes; per B the tile edge 256 / B and its neighbours (B = 1: 255 .. 257 are there already); four tiles, the span of one
# iteration of the kernel's loop, at B = 8
N_BINS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097) + (84, 85, 86) + (50, 51, 52) + (31, 32, 33) + (127, 128, 129)
RECEIVERS = (1, 3, 257)
CHANNELS = (1, 4)
VECTORS = (1, 2, GROUP - 1, GROUP, GROUP + 1, 31, 32)
WORDS = ("zero", "one", "max", "full", "decay", "single0", "single1", "single2", "single3")
COEFS = ("max", "min", "neg1", "zero", "alt", "altneg", "full", "ones", "index")
WEIGHTS = ("none", "zero", "max", "random")
MAX_ENTRIES = 1 << 20            # K x n_bins x B of a case
MAX_WORK = 1 << 23               # K x n_bins x B x J of a case: the reference stays well under a second
MAX32 = (1 << 32) - 1
I32_MAX, I32_MIN = (1 << 31) - 1, -(1 << 31)


def fits(n, B, K, J):
    return K * n * B <= MAX_ENTRIES and K * n * B * J <= MAX_WORK


def shapes():
    """(n_bins, B, K, channels, J) such that every pair of values of two of the five occurs in some shape that fits MAX_ENTRIES and
    MAX_WORK -- every pair but those that cannot (n_bins 4 097 with K 257 is 2^20 + 4 353 entries) -- built greedily and deterministically:
    the first uncovered pair fixes two values, each remaining one is chosen for the most pairs newly covered."""
    factors = (N_BINS, BANDS, RECEIVERS, CHANNELS, VECTORS)

    def ok(v):
        n, B, K, _, J = (v[f] if v[f] is not None else min(factors[f]) for f in range(5))
        return fits(n, B, K, J)

    todo = [((f, a), (h, b)) for f, h in combinations(range(5), 2) for a in factors[f] for b in factors[h]
            if ok([a if x == f else b if x == h else None for x in range(5)])]
    out = []
    while todo:
        (f, a), (h, b) = todo[0]
        v = [a if x == f else b if x == h else None for x in range(5)]
        for x in range(5):
            if v[x] is not None:
                continue
            best = None
            for cand in factors[x]:
                w = v[:x] + [cand] + v[x + 1:]
                if not ok(w):
                    continue
                gain = sum(1 for (p, pa), (q, qb) in todo if w[p] == pa and w[q] == qb)
                if best is None or gain > best[0]:
                    best = (gain, cand)
            v[x] = best[1]
        out.append(tuple(v))
        todo = [((p, pa), (q, qb)) for (p, pa), (q, qb) in todo if not (v[p] == pa and v[q] == qb)]
    return out


def words(kind, shape, rng, step):
    K, n, B = shape
    if kind == "zero":
        return np.zeros(shape, np.uint64)
    if kind == "one":
        return np.ones(shape, np.uint64)
    if kind == "max":
        return np.full(shape, (1 << 64) - 1, np.uint64)                    # a carry out of every 64-bit limb from the second bin on
    if kind == "full":
        return rng.integers(0, 1 << 64, shape, dtype=np.uint64)
    if kind == "decay":
        i = np.arange(n, dtype=np.float64).reshape(1, n, 1)
        return np.floor(2.0 ** 40 * 10.0 ** (-6.0 * i / n) * rng.uniform(0.5, 1.5, shape)).astype(np.uint64)
    # a single non-zero word: the first or last bin of the first or last tile
    tiles = (n + step - 1) // step
    at = (0, min(step, n) - 1, (tiles - 1) * step, n - 1)[int(kind[-1])]
    h = np.zeros(shape, np.uint64)
    h[rng.integers(K), at, rng.integers(B)] = rng.integers(1 << 62, 1 << 64, dtype=np.uint64)
    return h


def coefficients(kind, n, rng):
    i = np.arange(n, dtype=np.int64)
    if kind == "max":
        return np.full(n, I32_MAX, np.int64)
    if kind == "min":
        return np.full(n, I32_MIN, np.int64)
    if kind == "neg1":
        return np.full(n, -1, np.int64)
    if kind == "zero":
        return np.zeros(n, np.int64)
    if kind == "alt":
        return 1 - 2 * (i & 1)                                              # +1, -1, ...: equal words and an even n_bins cancel to exactly 0
    if kind == "altneg":
        return 2 * (i & 1) - 1                                              # -1, +1, ...: equal words and an odd n_bins leave minus one word
    if kind == "full":
        return rng.integers(I32_MIN, I32_MAX + 1, n, dtype=np.int64)
    if kind == "ones":
        return np.ones(n, np.int64)
    return i                                                                # c = i: the reduction's S1


class Case:
    def __init__(self, index, n_bins, B, K, channels, J, word=None, coef=None, weight=None):
        self.index, self.n_bins, self.B, self.K, self.channels, self.J = index, n_bins, B, K, channels, J
        self.word = WORDS[index % len(WORDS)] if word is None else word
        self.coef = index // 2 % len(COEFS) if coef is None else coef      # the class of vector 0; vector j has class coef + j
        self.weight_kind = WEIGHTS[index // 3 % len(WEIGHTS)] if weight is None else weight
        assert fits(n_bins, B, K, J), (n_bins, B, K, J)
        self.id = f"{index}-n{n_bins}-B{B}-K{K}-c{channels}-J{J}-{self.word}-{COEFS[self.coef % len(COEFS)]}-{self.weight_kind}"

    def coef_kinds(self):
        return [COEFS[(self.coef + j) % len(COEFS)] for j in range(self.J)]


@lru_cache(maxsize=None)
def inputs(case):
    """(hist [K, n_bins, B(, C)] uint64, coef [J, n_bins] int32, weight [n_bins, B] uint32 or None), from the case's seed.  With channels
    the words of the channels after W are random: they must not be read."""
    rng = np.random.default_rng(7000 + case.index)
    shape = (case.K, case.n_bins, case.B)
    w0 = words(case.word, shape, rng, 256 // case.B)
    if case.channels == 1:
        hist = w0
    else:
        hist = rng.integers(0, 1 << 64, shape + (case.channels,), dtype=np.uint64)
        hist[..., 0] = w0
    coef = np.stack([coefficients(kind, case.n_bins, rng) for kind in case.coef_kinds()]).astype(np.int32)
    wk = case.weight_kind
    weight = None if wk == "none" else (np.zeros((case.n_bins, case.B), np.uint32) if wk == "zero" else
                                        np.full((case.n_bins, case.B), MAX32, np.uint32) if wk == "max" else
                                        rng.integers(0, 1 << 32, (case.n_bins, case.B), dtype=np.uint64).astype(np.uint32))
    return hist, coef, weight


@lru_cache(maxsize=None)
def reference(case):
    hist, coef, weight = inputs(case)
    return project_ref(hist, coef, weight)


def sweep_case(seed):
    """A case drawn from the seed: any of the cover's values for each of the five, redrawn until it fits, and any classes."""
    rng = np.random.default_rng(90_000 + seed)
    while True:
        n, B, K, ch, J = (int(rng.choice(f)) for f in (N_BINS, BANDS, RECEIVERS, (1, 1, 4, 4, 9, 16), tuple(range(1, 33))))
        if fits(n, B, K, J):
            break
    return Case(5000 + seed, n, B, K, ch, J, word=WORDS[rng.integers(len(WORDS))], coef=int(rng.integers(len(COEFS))),
                weight=WEIGHTS[rng.integers(len(WEIGHTS))])


COVER = [Case(i, *s) for i, s in enumerate(shapes())]
# every word class with every weight at one shape that has idle threads (B = 3), a partial last tile and several tiles; nine vectors: every
# coefficient class in every case, two sweeps
CLASSES = [Case(1000 + 4 * a + b, 300, 3, 3, 1 + 3 * ((a + b) % 2), 9, word=w, coef=a, weight=x) for a, w in enumerate(WORDS) for b, x in enumerate(WEIGHTS)]
# 2^64 - 1 in every word against every coefficient class, unweighted: the largest sums of either sign (|P| near 2^103), and the exact zero
EXTREMES = [Case(1100, 300, 3, 3, 1, 9, word="max", coef=0, weight="none"), Case(1101, 301, 5, 1, 1, 9, word="max", coef=0, weight="none"),
            Case(1102, 300, 8, 3, 4, 9, word="one", coef=0, weight="none"), Case(1103, 301, 1, 3, 1, 9, word="one", coef=0, weight="none")]
# nine and sixteen channels: the words after W are garbage
HIGHER = [Case(1200, 257, 8, 3, 9, 9, word="full", coef=6, weight="random"), Case(1201, 65, 3, 3, 16, 5, word="decay", coef=4, weight="none")]
# the vector counts around the sweep group and its multiples, on several tiles with a partial last one
GROUPS = [Case(1300 + J, 257, 8, 3, 1, J, word="full", coef=J, weight=WEIGHTS[J % 4]) for J in (3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 23, 24, 25, 29, 31, 32)]
FIXED = COVER + CLASSES + EXTREMES + HIGHER + GROUPS
