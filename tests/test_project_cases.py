"""The cases of the projection's device tests (tests/project_cases.py) hold what they name, checked on the reference's own results
(tests/project_ref.py) without a GPU: the cover is pairwise and within its size limits, every class occurs with every weight, and among the
expected sums there are negative ones, exact zeros from non-zero inputs, non-trivial hi words of either sign and magnitudes of 2^100 and
more."""
from itertools import combinations

import numpy as np

from tests import project_cases as pc
from tests.project_ref import to_int


def test_the_cover_is_pairwise_and_within_the_limits():
    factors = (pc.N_BINS, pc.BANDS, pc.RECEIVERS, pc.CHANNELS, pc.VECTORS)
    seen = set()
    for c in pc.COVER:
        v = (c.n_bins, c.B, c.K, c.channels, c.J)
        assert c.K * c.n_bins * c.B <= 1 << 20
        for f, h in combinations(range(5), 2):
            seen.add((f, v[f], h, v[h]))
    missing = [(f, a, h, b) for f, h in combinations(range(5), 2) for a in factors[f] for b in factors[h] if (f, a, h, b) not in seen]
    assert missing == [(0, 4097, 2, 257)], missing                          # 4 097 x 257 bins alone exceed 2^20 entries
    for B in pc.BANDS:                                                       # the tile edge of every B and its neighbours
        assert {256 // B - 1, 256 // B, 256 // B + 1} <= set(pc.N_BINS)
    assert {pc.GROUP - 1, pc.GROUP, pc.GROUP + 1} <= set(pc.VECTORS) and {1, 2, 31, 32} <= set(pc.VECTORS)
    assert all(c.K * c.n_bins * c.B <= 1 << 20 for c in pc.FIXED)
    assert len({c.id for c in pc.FIXED}) == len(pc.FIXED)


def test_every_class_occurs_with_every_weight_and_every_channel_count():
    assert {(c.word, c.weight_kind) for c in pc.CLASSES} == {(w, x) for w in pc.WORDS for x in pc.WEIGHTS}
    for c in pc.CLASSES:
        assert set(c.coef_kinds()) == set(pc.COEFS)
    assert {c.channels for c in pc.FIXED} == {1, 4, 9, 16}
    assert {3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32} <= {c.J for c in pc.GROUPS}
    for c in pc.HIGHER:                                                      # the other channels' words are there, and they are not W's
        hist, _, _ = pc.inputs(c)
        assert hist.shape[3] == c.channels and (hist[..., 1:] != hist[..., :1]).any()
    for kind in ("single0", "single1", "single2", "single3"):
        c = next(x for x in pc.CLASSES if x.word == kind)
        hist, _, _ = pc.inputs(c)
        w = hist[..., 0] if hist.ndim == 4 else hist
        assert np.count_nonzero(w) == 1
        at = int(np.argwhere(w)[0][1])
        assert at == {"single0": 0, "single1": 84, "single2": 255, "single3": 299}[kind]          # n_bins 300, B 3: tiles of 85 bins


def test_the_expected_sums_hold_the_named_extremes():
    neg = zero = hi_pos = hi_neg = big = 0
    for c in pc.EXTREMES + pc.CLASSES[:12]:
        hist, coef, weight = pc.inputs(c)
        p = to_int(pc.reference(c))
        w = hist[..., 0] if hist.ndim == 4 else hist
        neg += int((p < 0).sum())
        hi_pos += int(((p >= 1 << 64)).sum())
        hi_neg += int((p < -(1 << 64)).sum())
        big += int((abs(p) >= 1 << 100).sum())
        if w.all() and weight is None:                                       # non-zero inputs ...
            for j in range(c.J):
                if coef[j].all():
                    zero += int((p[:, :, j] == 0).sum())                     # ... that cancel exactly
    assert neg > 0 and zero > 0 and hi_pos > 0 and hi_neg > 0 and big > 0, (neg, zero, hi_pos, hi_neg, big)
    # by hand: all words 1, n_bins 301, -1 +1 ... -1 leaves -1; n_bins 300, +1 -1 ... cancels
    c = pc.EXTREMES[3]
    j = c.coef_kinds().index("altneg")
    assert (to_int(pc.reference(c))[:, :, j] == -1).all()
    c = pc.EXTREMES[2]
    j = c.coef_kinds().index("alt")
    assert (to_int(pc.reference(c))[:, :, j] == 0).all()
    # 2^64 - 1 in 300 bins against INT32_MIN: -(2^64 - 1) * 300 * 2^31, about -2^103
    c = pc.EXTREMES[0]
    j = c.coef_kinds().index("min")
    assert (to_int(pc.reference(c))[:, :, j] == -((1 << 64) - 1) * 300 * (1 << 31)).all()


def test_sweep_cases_are_reproducible_and_fit():
    a, b = pc.sweep_case(3), pc.sweep_case(3)
    assert a.id == b.id and len({pc.sweep_case(s).id for s in range(50)}) == 50
    assert all(pc.fits(c.n_bins, c.B, c.K, c.J) for c in map(pc.sweep_case, range(50)))
