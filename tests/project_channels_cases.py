"""The cases of the device tests of the directional projection (tests/test_gpu_hist_project_channels.py): a pairwise cover of the shapes
-- every (B, channels) with every n_bins at the kernel's tile edges, every vector count around the sweep group, one and three receivers --
with the word, coefficient and weight classes dealt over them; fixed cases that hold every word class with every kind of weights, the
"negative weighted" cases on which a weighting that truncates towards zero differs from the definition's floor, and the idle-thread shape
(B = 7, channels = 9: 252 of 256 threads) with a non-zero last bin; sweep_case(seed) for a seeded sweep; inputs from a seed, and the
reference (tests/project_channels_ref.py) computed once per case.  A case holds fewer than MAX_WORDS = 2^22 histogram words.  No GPU, no
torch.  tests/test_project_channels_cases.py proves that the cases hold what they name."""
from functools import lru_cache
from itertools import combinations

import numpy as np

from tests.project_channels_ref import project_channels_ref
from tests.project_cases import COEFS, I32_MAX, I32_MIN, MAX32, coefficients  # noqa: F401  (the coefficient classes are the projection's)

# one tile (1, 2, 3), the tile edge 256 / (B x channels) for the pair counts 8 (31 .. 33), and for 1 (255 .. 257), several tiles with a
# ragged end (1000); for the other pair counts these are interior sizes of several tiles
N_BINS = (1, 2, 3, 31, 32, 33, 255, 256, 257, 1000)
PAIRS = tuple((B, ch) for B in range(1, 9) for ch in (1, 4, 9, 16))          # B x channels from 1 to 128: scan strides below, at and above a wave
RECEIVERS = (1, 3)
VECTORS = (1, 7, 8, 9, 17, 32)
WORDS = ("zero", "wmax", "min", "max", "neg1", "pos1", "alt", "full", "negsmall", "lastbin")
WEIGHTS = ("none", "zero", "one", "max", "random", "small")
MAX_WORDS = 1 << 22
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def pairwise(factors):
    """Tuples over the factors such that every pair of values of two factors occurs in one, built greedily and deterministically: the
    first uncovered pair fixes two values, each remaining one is chosen for the most pairs newly covered."""
    n = len(factors)
    todo = [((f, a), (h, b)) for f, h in combinations(range(n), 2) for a in factors[f] for b in factors[h]]
    out = []
    while todo:
        (f, a), (h, b) = todo[0]
        v = [a if x == f else b if x == h else None for x in range(n)]
        for x in range(n):
            if v[x] is not None:
                continue
            best = None
            for cand in factors[x]:
                w = v[:x] + [cand] + v[x + 1:]
                gain = sum(1 for (p, pa), (q, qb) in todo if w[p] == pa and w[q] == qb)
                if best is None or gain > best[0]:
                    best = (gain, cand)
            v[x] = best[1]
        out.append(tuple(v))
        todo = [((p, pa), (q, qb)) for (p, pa), (q, qb) in todo if not (v[p] == pa and v[q] == qb)]
    return out


def words(kind, shape, rng):
    """uint64 [K, n_bins, B, C]: channel 0 unsigned, the channels after it two's-complement int64 of the class `kind`."""
    K, n, B, C = shape
    h = np.zeros(shape, np.uint64)
    s = h[..., 1:].view(np.int64)                                            # the signed channels, written in place
    if kind == "zero":
        return h
    if kind == "wmax":
        h[..., 0] = np.uint64((1 << 64) - 1)                                 # a carry out of every 64-bit limb from the second bin on
        s[...] = rng.integers(I64_MIN, I64_MAX, s.shape, dtype=np.int64, endpoint=True)
    elif kind in ("min", "max", "neg1", "pos1"):
        h[..., 0] = rng.integers(0, 1 << 64, (K, n, B), dtype=np.uint64)
        s[...] = dict(min=I64_MIN, max=I64_MAX, neg1=-1, pos1=1)[kind]
    elif kind == "alt":
        h[..., 0] = np.uint64(1 << 63)
        big = rng.integers(1 << 61, 1 << 63, s.shape, dtype=np.int64)
        s[...] = big * (1 - 2 * ((np.arange(n).reshape(1, n, 1, 1) + np.arange(C - 1).reshape(1, 1, 1, C - 1)) & 1))
    elif kind == "full":
        h[...] = rng.integers(0, 1 << 64, shape, dtype=np.uint64)
    elif kind == "negsmall":
        h[..., 0] = rng.integers(0, 1 << 20, (K, n, B), dtype=np.uint64)
        s[...] = -rng.integers(1, 1 << 20, s.shape, dtype=np.int64)
    else:                                                                    # lastbin: every word of the last bin, nothing else
        h[:, n - 1, :, 0] = rng.integers(1 << 62, 1 << 64, (K, B), dtype=np.uint64)
        s[:, n - 1] = rng.integers(I64_MIN, I64_MAX, s[:, n - 1].shape, dtype=np.int64, endpoint=True)
    return h


def weights(kind, n, B, rng):
    if kind == "none":
        return None
    if kind in ("zero", "one", "max"):
        return np.full((n, B), dict(zero=0, one=1, max=MAX32)[kind], np.uint32)
    hi = 1 << 32 if kind == "random" else 5                                  # small: 1 .. 4
    return rng.integers(kind == "small", hi, (n, B), dtype=np.uint64).astype(np.uint32)


class Case:
    def __init__(self, index, n_bins, B, channels, K, J, word=None, coef=None, weight=None):
        self.index, self.n_bins, self.B, self.channels, self.K, self.J = index, n_bins, B, channels, K, J
        self.word = WORDS[index % len(WORDS)] if word is None else word
        self.coef = index // 2 % len(COEFS) if coef is None else coef      # the class of vector 0; vector j has class coef + j
        self.weight_kind = WEIGHTS[index // 3 % len(WEIGHTS)] if weight is None else weight
        assert K * n_bins * B * channels < MAX_WORDS
        self.id = f"{index}-n{n_bins}-B{B}-c{channels}-K{K}-J{J}-{self.word}-{COEFS[self.coef % len(COEFS)]}-{self.weight_kind}"

    def coef_kinds(self):
        return [COEFS[(self.coef + j) % len(COEFS)] for j in range(self.J)]

    @property
    def device(self):
        """A fifth of the cases go through the _device call with guard words behind the output."""
        return self.index % 5 == 0


@lru_cache(maxsize=None)
def inputs(case):
    """(hist [K, n_bins, B, C] uint64 -- [K, n_bins, B] with one channel --, coef [J, n_bins] int32, weight [n_bins, B] uint32 or None)."""
    rng = np.random.default_rng(8000 + case.index)
    hist = words(case.word, (case.K, case.n_bins, case.B, case.channels), rng)
    if case.channels == 1:
        hist = np.ascontiguousarray(hist[..., 0])
    coef = np.stack([coefficients(kind, case.n_bins, rng) for kind in case.coef_kinds()]).astype(np.int32)
    return hist, coef, weights(case.weight_kind, case.n_bins, case.B, rng)


@lru_cache(maxsize=None)
def reference(case):
    hist, coef, weight = inputs(case)
    return project_channels_ref(hist, coef, weight)


def sweep_case(seed):
    """A case drawn from the seed: any of the cover's values for each factor and any classes."""
    rng = np.random.default_rng(91_000 + seed)
    n, (B, ch), K, J = (f[rng.integers(len(f))] for f in (N_BINS, PAIRS, RECEIVERS, tuple(range(1, 33))))
    return Case(5000 + seed, int(n), B, ch, int(K), int(J), word=WORDS[rng.integers(len(WORDS))], coef=int(rng.integers(len(COEFS))),
                weight=WEIGHTS[rng.integers(len(WEIGHTS))])


COVER = [Case(i, n, B, ch, K, J) for i, (n, (B, ch), K, J) in enumerate(pairwise((N_BINS, PAIRS, RECEIVERS, VECTORS)))]
# every word class with every kind of weights at one shape with idle threads (B = 3, nine channels: 27 pairs, 243 threads), several tiles
# and a ragged end; nine vectors: every coefficient class in every case, two sweeps
CLASSES = [Case(1000 + len(WEIGHTS) * a + b, 40, 3, 9, 3, 9, word=w, coef=a, weight=x) for a, w in enumerate(WORDS) for b, x in enumerate(WEIGHTS)]
# "negative weighted": a negative word times a small weight, where floor and truncation part; vector 0 is ones (no cancellation), h = -1
# and w = 1 first
NEGATIVE_WEIGHTED = [Case(1100, 5, 1, 4, 1, 1, word="neg1", coef=7, weight="one"), Case(1101, 33, 2, 4, 3, 3, word="negsmall", coef=7, weight="small"),
                     Case(1102, 257, 5, 9, 1, 9, word="negsmall", coef=7, weight="random"), Case(1103, 64, 8, 16, 3, 8, word="alt", coef=7, weight="small"),
                     Case(1104, 40, 7, 9, 1, 2, word="neg1", coef=7, weight="small")]
# the idle-thread shape: B = 7 with nine channels is 63 pairs, a tile of four bins on 252 threads; the last bin alone is non-zero, on the
# last tile's every position (n_bins = 4 m + 1 .. 4 m + 4)
IDLE = [Case(1200 + r, 36 + r, 7, 9, 3, 9, word="lastbin", coef=6, weight=WEIGHTS[r]) for r in range(1, 5)]
FIXED = COVER + CLASSES + NEGATIVE_WEIGHTED + IDLE
