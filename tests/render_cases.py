"""The cases of the tests of the rendering (tests/test_render_cases.py on the reference alone, tests/test_gpu_render.py on the device): a
case type, fixed cases that name the class they stand for, and a seeded sweep over the whole parameter space; inputs from a seed, and the
reference (tests/render_ref.py) computed once per case.  Shapes keep K * B * N * T <= 2^24, so a reference takes well under a second.
No GPU, no torch."""
from functools import lru_cache

import numpy as np

from tests.render_ref import render_ref

U64 = (1 << 64) - 1
INT64_MIN = 1 << 63                                  # as the uint64 word that holds it
CHANNELS = (1, 4, 9, 16)


class Case:
    """words: how the W words are filled -- "random", or an int (every W word is that value).  signed: how the channel words are filled
    -- "random" (|hc| <= hW), "negative" (every word negative), "int64_min" (every word INT64_MIN).  weight: "none", "random", "kills" (a
    weight of 1: g = 0 for every h < 2^32).  taps: "random", "one" (B = T = 1, [1.0]), "zero_band" (band 0 all zero), "negative" (every
    tap < 0), "denormal" (denormal taps among normal ones)."""

    def __init__(self, cls, index, K=2, n_bins=5, B=3, channels=4, M=3, T=7, frac_bits=20, seed=12345, words="random", signed="random",
                 weight="none", taps="random"):
        self.cls, self.index = cls, index
        self.K, self.n_bins, self.B, self.channels, self.M, self.T = K, n_bins, B, channels, M, T
        self.frac_bits, self.seed, self.words, self.signed, self.weight, self.taps = frac_bits, seed, words, signed, weight, taps
        assert K * B * n_bins * M * T <= 1 << 24, cls
        self.id = f"{index}-{cls}-K{K}-n{n_bins}-B{B}-c{channels}-M{M}-T{T}"

    @property
    def N(self):
        return self.n_bins * self.M


@lru_cache(maxsize=None)
def inputs(case):
    """(hist uint64 [K, n_bins, B, channels] -- [K, n_bins, B] for one channel --, weight uint32 [n_bins, B] or None, taps float64 [B, T])."""
    rng = np.random.default_rng(7000 + case.index)
    K, nb, B, C = case.K, case.n_bins, case.B, case.channels
    if case.words == "random":
        W = rng.integers(0, 1 << 44, (K, nb, B), dtype=np.uint64) * (rng.integers(0, 8, (K, nb, B), dtype=np.uint64) != 0)      # an eighth empty
    else:
        W = np.full((K, nb, B), case.words, np.uint64)
    hist = np.zeros((K, nb, B, C), np.uint64)
    hist[..., 0] = W
    if C > 1:
        if case.signed == "random":
            f = rng.uniform(-1.0, 1.0, (K, nb, B, C - 1))
            hist[..., 1:] = np.trunc(f * np.minimum(W, 1 << 62).astype(np.float64)[..., None]).astype(np.int64).view(np.uint64)
        elif case.signed == "negative":
            hist[..., 1:] = (-rng.integers(1, 1 << 40, (K, nb, B, C - 1), dtype=np.int64)).view(np.uint64)
        else:
            hist[..., 1:] = INT64_MIN
    weight = None
    if case.weight == "random":
        weight = rng.integers(0, 1 << 32, (nb, B), dtype=np.uint64).astype(np.uint32)
    elif case.weight == "kills":
        weight = np.ones((nb, B), np.uint32)
    if case.taps == "one":
        taps = np.ones((1, 1))
    else:
        taps = rng.uniform(-1.0, 1.0, (B, case.T))
        if case.taps == "zero_band":
            taps[0] = 0.0
        elif case.taps == "negative":
            taps = -np.abs(taps) - 2.0 ** -20
        elif case.taps == "denormal":
            taps[:, ::2] = rng.integers(1, 1 << 40, taps[:, ::2].shape).astype(np.float64) * 5e-324 * rng.choice([-1.0, 1.0], taps[:, ::2].shape)
    return (hist[..., 0] if C == 1 else hist), weight, np.ascontiguousarray(taps)


@lru_cache(maxsize=None)
def reference(case):
    hist, weight, taps = inputs(case)
    out = render_ref(hist, taps, case.M, case.frac_bits, case.seed, weight)
    out.flags.writeable = False
    return out


def _fixed():
    c, n = [], [0]

    def add(cls, **kw):
        c.append(Case(cls, n[0], **kw))
        n[0] += 1

    add("T=1", T=1)
    add("T>M", T=100, M=3, n_bins=40)                                        # the halo spans 33 bins
    add("T=1024", T=1024, M=64, n_bins=4, B=8, channels=1, K=1)              # 64 KiB of taps
    add("T=1024,M=1024", T=1024, M=1024, n_bins=1, B=8, channels=16, K=1)    # the largest tile: one bin, 64 KiB of samples
    for M in (1, 3, 64, 65):
        add(f"M={M}", M=M, n_bins=9, T=33)
    add("M=1024", M=1024, n_bins=2, T=33, B=8, K=1)
    for total, (nb, M, T) in ((63, (8, 7, 8)), (64, (8, 7, 9)), (65, (8, 7, 10)), (255, (16, 15, 16)), (256, (16, 15, 17)), (257, (16, 15, 18)),
                              (1025, (32, 31, 34))):
        assert nb * M + T - 1 == total
        add(f"N+T-1={total}", n_bins=nb, M=M, T=T)
    for B in (1, 3, 8):
        add(f"B={B}", B=B, M=16, n_bins=11, T=31)
    for C in CHANNELS:
        add(f"channels={C}", channels=C, B=8, M=5, n_bins=33)
    for K in (1, 2, 257):
        add(f"K={K}", K=K, B=2, n_bins=3, M=5, T=9)
    for name, w in (("0", 0), ("1", 1), ("2^53+1", (1 << 53) + 1), ("2^64-1", U64)):
        add(f"word={name}", words=w, frac_bits=0 if w <= 1 else 30)
    add("weight kills", words=5, weight="kills")
    add("weight", weight="random", M=16, n_bins=40, B=8)
    add("negative words", signed="negative")
    add("INT64_MIN", signed="int64_min", channels=16)
    add("hW=0", words=0, signed="negative", channels=9)
    add("zero filter", taps="zero_band")
    add("negative taps", taps="negative")
    add("denormal taps", taps="denormal")
    add("unit filter", taps="one", B=1, T=1, M=48, n_bins=30, channels=1, K=3)
    add("frac_bits=0", frac_bits=0)
    add("frac_bits=62", frac_bits=62)
    add("seed=0", seed=0)
    add("seed=2^64-1", seed=U64)
    add("several tiles", M=240, n_bins=9, B=8, T=65, channels=16, K=2)       # tiles of two bins and a last tile of one
    return c


def _sweep(count=50):
    """The whole parameter space from one seed, shapes capped at K * B * N * T <= 2^24."""
    rng = np.random.default_rng(20240)
    c = []
    for x in range(count):
        while True:
            K = int(rng.choice([1, 2, 3, 5, 17]))
            B = int(rng.integers(1, 9))
            M = int(rng.choice([1, 2, 7, 16, 63, 64, 65, 100, 240, 511, 1024]))
            T = int(rng.choice([1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 255, 511, 1024]))
            nb = int(rng.integers(1, 41))
            if K * B * nb * M * T <= 1 << 24:
                break
        c.append(Case("sweep", 100 + x, K=K, n_bins=nb, B=B, channels=int(rng.choice(CHANNELS)), M=M, T=T, frac_bits=int(rng.integers(0, 63)),
                      seed=int(rng.integers(0, 1 << 64, dtype=np.uint64)), weight=str(rng.choice(["none", "random"])),
                      signed=str(rng.choice(["random", "negative"])), taps=str(rng.choice(["random", "negative", "denormal", "zero_band"]))))
    return c


FIXED = _fixed()
SWEEP = _sweep()
BY_CLASS = {c.cls: c for c in FIXED}
