"""The restatement of the directional projection (tests/project_channels_ref.py) and the cases of its device tests
(tests/project_channels_cases.py), checked without a GPU: the definition word for word and its vectorised form agree on every fixed case
small enough for the former; the column ch = 0 is the projection's restatement (tests/project_ref.py) and one channel is it entirely; the
weighting floors towards minus infinity (h = -1, w = 1 gives -1), and a weighting that truncates towards zero differs on every case marked
"negative weighted"; the cover is pairwise, and every class the device tests name is present in the inputs and in the expected sums."""
from itertools import combinations

import numpy as np

from tests import project_channels_cases as pc
from tests.project_channels_ref import project_channels_direct, project_channels_ints, project_channels_ref, to_int
from tests.project_ref import project_ref

DIRECT_MAX = 1 << 14                                                          # words x vectors a case may hold for the word-for-word form


def small(c):
    return c.K * c.n_bins * c.B * c.channels * c.J <= DIRECT_MAX


def test_the_two_restatements_agree_on_every_small_fixed_case():
    cases = [c for c in pc.FIXED if small(c)]
    assert len(cases) >= 60 and {c.channels for c in cases} == {1, 4, 9, 16}
    assert {c.word for c in cases} == set(pc.WORDS) and {c.weight_kind for c in cases} == set(pc.WEIGHTS)
    for c in cases:
        hist, coef, weight = pc.inputs(c)
        a, b = project_channels_direct(hist, coef, weight), pc.reference(c)
        assert a.dtype == b.dtype == np.uint64 and a.shape == b.shape == (c.K, c.B, c.J, c.channels, 2), c.id
        assert np.array_equal(a, b), c.id
        assert (to_int(b) == project_channels_ints(hist, coef, weight)).all(), c.id


def test_column_zero_is_the_projection_and_one_channel_is_it_entirely():
    seen = set()
    for c in pc.FIXED:
        if (c.channels, c.weight_kind) in seen or c.K * c.n_bins * c.B * c.channels > 1 << 16:
            continue
        seen.add((c.channels, c.weight_kind))
        hist, coef, weight = pc.inputs(c)
        want = project_ref(hist, coef, weight)                               # reads W alone
        assert np.array_equal(pc.reference(c)[:, :, :, 0], want), c.id
        if c.channels == 1:
            assert pc.reference(c).shape == want.shape[:3] + (1, 2)
    assert seen == {(ch, w) for ch in (1, 4, 9, 16) for w in pc.WEIGHTS}


def test_the_weighting_floors_towards_minus_infinity():
    h = np.zeros((1, 1, 1, 4), np.uint64)
    h[..., 0] = 7
    h[..., 1:].view(np.int64)[...] = (-1, 1, -(1 << 32) - 1)
    one = np.ones((1, 1), np.int32)
    w = np.ones((1, 1), np.uint32)
    for f in (project_channels_direct, project_channels_ref):
        assert to_int(f(h, one, w)).reshape(-1).tolist() == [0, -1, 0, -2]                       # 7 >> 32, -1 >> 32, 1 >> 32, (-2^32 - 1) >> 32
        assert to_int(f(h, one, w, truncating=True)).reshape(-1).tolist() == [0, 0, 0, -1]       # not the definition
        assert to_int(f(h, one)).reshape(-1).tolist() == [7, -1, 1, -(1 << 32) - 1]
        assert to_int(f(h, -one)).reshape(-1).tolist() == [-7, 1, -1, (1 << 32) + 1]
    # the case with h = -1 and w = 1: five bins of ones against -1 give -5 per signed channel
    c = pc.NEGATIVE_WEIGHTED[0]
    hist, coef, weight = pc.inputs(c)
    assert (hist[..., 1:].view(np.int64) == -1).all() and (weight == 1).all() and (coef == 1).all()
    assert (to_int(pc.reference(c))[..., 1:] == -5).all()
    for c in pc.NEGATIVE_WEIGHTED:                                            # a truncating restatement must differ on each of them
        hist, coef, weight = pc.inputs(c)
        assert c.channels > 1 and weight is not None and (hist[..., 1:].view(np.int64) < 0).any()
        wrong = project_channels_ref(hist, coef, weight, truncating=True)
        assert not np.array_equal(wrong, pc.reference(c)), c.id
        assert np.array_equal(wrong[..., 0, :], pc.reference(c)[..., 0, :]), c.id                # W is unsigned: the same either way
        if small(c):
            assert np.array_equal(wrong, project_channels_direct(hist, coef, weight, truncating=True)), c.id


def test_the_cover_is_pairwise_and_within_the_limit():
    factors = (pc.N_BINS, pc.PAIRS, pc.RECEIVERS, pc.VECTORS)
    seen = set()
    for c in pc.COVER:
        v = (c.n_bins, (c.B, c.channels), c.K, c.J)
        for f, h in combinations(range(4), 2):
            seen.add((f, v[f], h, v[h]))
    assert not [(f, a, h, b) for f, h in combinations(range(4), 2) for a in factors[f] for b in factors[h] if (f, a, h, b) not in seen]
    assert set(pc.PAIRS) == {(B, ch) for B in range(1, 9) for ch in (1, 4, 9, 16)}
    assert {B * ch for B, ch in pc.PAIRS} >= {1, 32, 63, 64, 72, 128}         # the scan stride below, at and above a wave
    assert set(pc.N_BINS) == {1, 2, 3, 31, 32, 33, 255, 256, 257, 1000} and set(pc.VECTORS) == {1, 7, 8, 9, 17, 32}
    assert all(c.K * c.n_bins * c.B * c.channels < 1 << 22 for c in pc.FIXED)
    assert len({c.id for c in pc.FIXED}) == len(pc.FIXED)
    assert len(pc.COVER) // 6 <= sum(c.device for c in pc.COVER) <= len(pc.COVER) // 4           # a fifth through the _device call


def test_every_named_class_is_present():
    assert {(c.word, c.weight_kind) for c in pc.CLASSES} == {(w, x) for w in pc.WORDS for x in pc.WEIGHTS}
    for c in pc.CLASSES:
        assert set(c.coef_kinds()) == set(pc.COEFS) and c.channels == 9
    by_word = {c.word: pc.inputs(c)[0] for c in pc.CLASSES if c.weight_kind == "none"}
    s = {k: v[..., 1:].view(np.int64) for k, v in by_word.items()}
    assert not by_word["zero"].any()
    assert (by_word["wmax"][..., 0] == np.uint64((1 << 64) - 1)).all()
    assert (s["min"] == pc.I64_MIN).all() and (s["max"] == pc.I64_MAX).all() and (s["neg1"] == -1).all() and (s["pos1"] == 1).all()
    assert ((s["alt"][:, :-1] < 0) != (s["alt"][:, 1:] < 0)).all()            # the sign alternates from bin to bin
    assert (s["full"] < 0).any() and (s["full"] > 0).any()
    assert (s["negsmall"] < 0).all() and (s["negsmall"] > -(1 << 20)).all()
    coefs = np.concatenate([pc.inputs(c)[1].reshape(-1) for c in pc.CLASSES[:6]])
    assert {pc.I32_MIN, pc.I32_MAX, 0, 1, -1} <= set(coefs.tolist()) and len(set(coefs.tolist())) > 100
    kinds = {c.weight_kind: pc.inputs(c)[2] for c in pc.CLASSES[:6]}
    assert kinds["none"] is None and not kinds["zero"].any() and (kinds["one"] == 1).all() and (kinds["max"] == pc.MAX32).all()
    assert len(set(kinds["random"].reshape(-1).tolist())) > 50 and set(kinds["small"].reshape(-1).tolist()) == {1, 2, 3, 4}
    # the idle-thread shape: 63 pairs, a tile of four bins on 252 threads; only the last bin holds anything, on each position of a tile
    assert {(c.B, c.channels) for c in pc.IDLE} == {(7, 9)} and {c.n_bins % 4 for c in pc.IDLE} == {0, 1, 2, 3}
    for c in pc.IDLE:
        hist = pc.inputs(c)[0]
        assert hist[:, -1].all() and not hist[:, :-1].any()
    # among the expected sums: negative ones, non-trivial hi words of either sign, magnitudes of 2^100 and more, in signed channels too
    neg = hi_pos = hi_neg = big = 0
    for c in pc.CLASSES[6:30]:
        p = to_int(pc.reference(c))[..., 1:]
        neg += int((p < 0).sum())
        hi_pos += int((p >= 1 << 64).sum())
        hi_neg += int((p < -(1 << 64)).sum())
        big += int((abs(p) >= 1 << 98).sum())
    assert neg > 0 and hi_pos > 0 and hi_neg > 0 and big > 0, (neg, hi_pos, hi_neg, big)
    # by hand: INT64_MIN in 40 bins against INT32_MIN is 40 * 2^94
    c = next(x for x in pc.CLASSES if x.word == "min" and x.weight_kind == "none")
    j = c.coef_kinds().index("min")
    assert (to_int(pc.reference(c))[:, :, j, 1:] == 40 << 94).all()


def test_sweep_cases_are_reproducible_and_fit():
    a, b = pc.sweep_case(3), pc.sweep_case(3)
    assert a.id == b.id and len({pc.sweep_case(s).id for s in range(50)}) == 50
    assert {pc.sweep_case(s).channels for s in range(50)} == {1, 4, 9, 16}
