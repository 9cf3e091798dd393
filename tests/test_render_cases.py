"""The rendering's cases and its restatement (tests/render_cases.py, tests/render_ref.py) without a GPU: every fixed case holds the class
it names; the unit filter gives |out| = sqrt(e / M) exactly and the bin's energy within M * 2^-52; channel 0 of a 16-channel histogram
is the render of its W words alone; the references are pinned by digest (tests/golden/render_reference_digests.json); and band_taps
telescopes to the unit impulse."""
import hashlib
import json
import os

import numpy as np
import pytest

import hare_amd as H
from tests.render_cases import BY_CLASS, FIXED, INT64_MIN, SWEEP, U64, inputs, reference
from tests.render_ref import render_ref, signs, weighted

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_reference_digests.json")


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def W_of(hist):
    return hist if hist.ndim == 3 else hist[..., 0]


def holds(case):
    """Whether the case is of the class it names: a statement about its parameters, its inputs and, where the class is about a result,
    its reference."""
    hist, weight, taps = inputs(case)
    out = reference(case)
    cls, W = case.cls, W_of(hist)
    key, _, val = cls.partition("=")
    if key in ("T", "M", "B", "channels", "K", "frac_bits") and val.isdigit():
        return getattr(case, key) == int(val) and out.any()
    if cls == "T>M":
        return case.T - 1 > 2 * case.M and out.any()
    if cls == "T=1024,M=1024":
        return case.T == 1024 and case.M == 1024 and out.any()
    if key == "N+T-1":
        return case.N + case.T - 1 == int(val) and out.any()
    if key == "word":
        want = {"0": 0, "1": 1, "2^53+1": (1 << 53) + 1, "2^64-1": U64}[val]
        rounds = float(want) != want if want else False
        return (W == np.uint64(want)).all() and (out.any() == (want != 0)) and (val != "2^53+1" or rounds)
    if cls == "weight kills":
        return W.all() and not weighted(W, weight).any() and not out.any()
    if cls == "weight":
        g = weighted(W, weight)
        return weight is not None and (g < W).any() and g.any() and out.any()
    if cls == "negative words":
        return (hist[..., 1:].view(np.int64) < 0).all() and (out[:, 1:] != 0).any()
    if cls == "INT64_MIN":
        return (hist[..., 1:] == np.uint64(INT64_MIN)).all() and W.any() and np.isfinite(out).all() and (out[:, 1:] != 0).any()
    if cls == "hW=0":
        return not W.any() and hist[..., 1:].all() and not out.any()
    if cls == "zero filter":
        return not taps[0].any() and taps[1:].any() and out.any()
    if cls == "negative taps":
        return (taps < 0).all() and out.any()
    if cls == "denormal taps":
        tiny = (taps != 0) & (np.abs(taps) < 2.0 ** -1022)
        return tiny.any() and (~tiny).any() and out.any()
    if cls == "unit filter":
        return case.B == 1 and case.T == 1 and taps.tolist() == [[1.0]]
    if key == "seed":
        return case.seed == {"0": 0, "2^64-1": U64}[val] and out.any()
    if cls == "several tiles":
        return case.n_bins * case.M > 2 * 4096 // case.B and case.T > 1 and out.any()
    return False


@pytest.mark.parametrize("case", FIXED, ids=lambda c: c.id)
def test_every_fixed_case_holds_the_class_it_names(case):
    assert holds(case), case.id


def test_the_fixed_cases_cover_what_the_device_test_is_to_meet():
    names = set(BY_CLASS)
    for want in ("T=1", "T>M", "T=1024", "M=1", "M=3", "M=64", "M=65", "M=1024", "B=1", "B=3", "B=8", "channels=1", "channels=4", "channels=9",
                 "channels=16", "K=1", "K=2", "K=257", "word=0", "word=1", "word=2^53+1", "word=2^64-1", "weight kills", "negative words",
                 "INT64_MIN", "hW=0", "zero filter", "negative taps", "denormal taps", "frac_bits=0", "frac_bits=62", "seed=0", "seed=2^64-1"):
        assert want in names, want
    assert {f"N+T-1={n}" for n in (63, 64, 65, 255, 256, 257, 1025)} <= names
    assert len(SWEEP) == 50 and len({c.id for c in FIXED + SWEEP}) == len(FIXED) + len(SWEEP)
    assert {c.channels for c in SWEEP} == {1, 4, 9, 16} and {c.B for c in SWEEP} == set(range(1, 9))


def test_signs_are_plus_or_minus_one_and_differ_between_receivers():
    s = signs(0, 3, 4096)
    assert set(np.unique(s).tolist()) == {-1.0, 1.0}
    assert abs(s.mean()) < 0.05 and abs((s[0] * s[1]).mean()) < 0.05          # 4 096 fair signs: |mean| below 3.2 sigma = 0.05
    assert not np.array_equal(s[0], s[1]) and np.array_equal(signs(0, 3, 100), s[:, :100])


def test_unit_filter_gives_the_bin_energy():
    """B = 1, T = 1, taps = [1.0]: y = +-1, p = M exactly (a sum of M ones), so a = sqrt(e / M) and |out| = a in every sample of the bin.
    The bin's energy is M correctly rounded products and M - 1 correctly rounded adds.  a * a carries half an ulp of the division halved by
    the root, half an ulp of the root doubled by the square and half an ulp of the product: 3.5 * 2^-53 relative; each add of the
    non-negative terms adds at most 2^-53: (M + 2.5) * 2^-53 in all, below M * 2^-52 from M = 3 on (here M = 48)."""
    case = BY_CLASS["unit filter"]
    hist, _, _ = inputs(case)
    out = reference(case)
    M = case.M
    e = np.ldexp(hist.astype(np.float64), -case.frac_bits)[..., 0]          # [K, n_bins]
    assert np.array_equal(np.abs(out[:, 0]).reshape(case.K, case.n_bins, M), np.repeat(np.sqrt(e / M)[..., None], M, axis=2))
    energy = (out[:, 0].reshape(case.K, case.n_bins, M) ** 2).sum(axis=2)
    assert (e > 0).any()
    assert (np.abs(energy - e) <= M * 2.0 ** -52 * e).all()


def test_channel_0_is_the_render_of_the_W_words_alone():
    case = BY_CLASS["channels=16"]
    hist, weight, taps = inputs(case)
    alone = render_ref(np.ascontiguousarray(hist[..., 0]), taps, case.M, case.frac_bits, case.seed, weight)
    assert alone.shape[1] == 1 and reference(case)[:, 0].tobytes() == alone[:, 0].tobytes()


def test_references_are_pinned_by_digest():
    want = json.load(open(GOLDEN))
    assert all(np.isfinite(reference(c)).all() for c in FIXED + SWEEP)       # the device test's poison is a NaN: no reference may hold one
    got = {c.id: digest(reference(c)) for c in FIXED + SWEEP}
    assert sorted(got) == sorted(want)
    assert [k for k in got if got[k] != want[k]] == []


def test_band_taps_telescope_to_the_unit_impulse():
    """The bands are differences of consecutive lowpasses, the last against the unit impulse: their sum is the impulse but for at most B
    roundings of values <= 1 each (about 1e-15); 1e-12 leaves room for the window arithmetic."""
    for fs, edges, T in ((48000.0, [88, 177, 354, 707, 1414, 2828, 5657], 511), (44100.0, [500.0], 33), (8000.0, [], 1), (16000.0, [1000, 2000], 1023)):
        taps = H.band_taps(fs, edges, T)
        assert taps.shape == (len(edges) + 1, T) and taps.dtype == np.float64 and np.isfinite(taps).all()
        delta = np.zeros(T)
        delta[(T - 1) // 2] = 1.0
        assert np.abs(taps.sum(axis=0) - delta).max() <= 1e-12
        if edges:
            assert abs(taps[0].sum() - 1.0) <= 1e-12 and np.abs(taps[1:].sum(axis=1)).max() <= 1e-12        # gains at 0 Hz: 1, then 0
    for bad in (dict(T=32), dict(T=0), dict(edges=[2000, 1000]), dict(edges=[30000]), dict(edges=[0.0])):
        with pytest.raises(ValueError):
            H.band_taps(**{**dict(fs=48000.0, edges=[1000], T=31), **bad})
