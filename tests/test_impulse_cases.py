"""The impulses' cases and their restatement (tests/impulse_cases.py, tests/impulse_ref.py) without a GPU: the references are pinned by
digest (tests/golden/impulse_reference_digests.json, NaNs canonicalised); a window of the reference is that window of the whole, and a
receiver of it that receiver alone; a single entry gives exactly gain * tap; two paths in one sample and band add as energies; the bands
descending, or the bins descending, differ from the definition on every plain-normal case whose sums could show it -- so a kernel that
walked the other way could not pass tests/test_gpu_impulses.py --; and every class the list names is present in it."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests.convolve_ref import canonical
from tests.impulse_cases import CASES, CHUNK, FIXED, INT64_MIN, SENTINEL, SWEEP, TILE, entry_count, inputs, plan, reference
from tests.impulse_ref import entries, gains, impulse_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "impulse_reference_digests.json")


def digest(y):
    return hashlib.sha256(np.ascontiguousarray(canonical(y)).tobytes()).hexdigest()


def whole(case, **kw):
    x = inputs(case)
    return impulse_ref(x["hist"], x["taps"], case.frac_bits, weight=x["weight"], **kw)


def test_the_references_are_pinned():
    have = {c.id: digest(reference(c)) for c in CASES}
    if os.environ.get("HARE_WRITE_GOLDEN") == "impulses":
        with open(GOLDEN, "w") as f:
            json.dump(have, f, indent=0, sort_keys=True)
    want = json.load(open(GOLDEN))
    assert set(want) == set(have)
    assert [k for k in have if have[k] != want[k]] == []


def test_the_list_follows_the_kernels_plan():
    assert (TILE, CHUNK) == (256, 256)
    assert plan(3, 8, 16, 1024, 257) == (6, 256, 8 * 8192 + 256 * 148 + 16) and plan(1, 1, 1, 1, 256) == (1, 256, 8 + 256 * 28 + 16)
    assert len(SWEEP) == 50 and len({c.id for c in CASES}) == len(CASES)


def test_every_class_named_is_present():
    F = FIXED
    assert {c.T for c in F} >= {1, 2, 33, 1024} and {c.n_bins for c in F} >= {1, 63, 64, 65, 255, 256, 257, 1025}
    assert {(c.T, c.n_bins) for c in F} >= {(T, nb) for T in (1, 2, 33, 1024) for nb in (1, 63, 64, 65, 255, 256, 257, 1025)}
    assert {c.C for c in F} == {1, 4, 9, 16} and {c.B for c in F} >= {1, 3, 8} and {c.K for c in F} >= {1, 3, 257}
    by = {c.name: c for c in F}
    assert entry_count(by["none"]) == 0 and not reference(by["none"]).view(np.uint64).any()          # every output +0.0
    for name, at in (("first", 0), ("last", 599), ("chunk-", CHUNK - 1), ("chunk+", CHUNK), ("tile-", TILE - 1), ("tile+", TILE)):
        c = by["one-" + name]
        assert c.positions() == [(at, 1)] and entry_count(c) == 1 and c.T > 1
    assert [i for i, _ in by["one-chunk-of-tile-1"].positions()] == [TILE - 32 + CHUNK - 1, TILE - 32 + CHUNK]       # tile 1 scans from TILE - (T - 1)
    (i0, b0), (i1, b1) = by["two-one-band"].positions()
    assert b0 == b1 and 0 < i1 - i0 < by["two-one-band"].T
    (i0, b0), (i1, b1) = by["two-bands"].positions()
    assert b0 > b1 and 0 < i1 - i0 < by["two-bands"].T          # the later bin in the earlier band: bands outer, not bins
    for name in ("dense", "dense-16"):
        assert by[name].n_bins == 300 and entry_count(by[name]) == by[name].K * 300 * by[name].B
    c = by["weight-empties"]
    x = inputs(c)
    (i0, b0), (i1, b1) = c.positions()[:2]
    g = entries(x["hist"], x["weight"])
    assert x["hist"][0, i0, b0, 0] != 0 and g[0, i0, b0] == 0 and g[0, i1, b1] == x["hist"][0, i1, b1, 0] >> np.uint64(32)
    for name in ("words-edge", "words-edge-16", "frac-62"):
        x = inputs(by[name])
        assert {1, (1 << 53) + 1, (1 << 64) - 1} <= set(int(v) for v in np.unique(x["hist"][..., 0]))
        sub = x["hist"][..., 1:].view(np.int64)
        assert (sub < 0).any() and (sub == INT64_MIN).any()
    assert by["frac-0"].frac_bits == 0 and by["frac-62"].frac_bits == 62
    t = {k: inputs(by["taps-" + k])["taps"] for k in ("negative", "denormal", "huge", "inf", "nan")}
    assert (t["negative"] < 0).all() and (np.abs(t["denormal"]) < 2.3e-308).all() and (t["denormal"] != 0).all()
    assert (np.abs(t["huge"]) > 2.0 ** 499).any() and (np.abs(t["huge"]) < 2.0 ** -499).any()
    assert np.isinf(t["inf"]).sum() == 1 and np.isnan(t["nan"]).sum() == 1 and by["taps-inf"].device_only and by["taps-nan"].device_only
    assert not any(c.device_only for c in CASES if c.taps not in ("inf", "nan"))
    assert np.isinf(reference(by["taps-inf"])).any() and np.isfinite(reference(by["taps-inf"])).any()          # it reaches some outputs, not all
    assert {c.window for c in F} == {"whole", "one", "head", "tail", "tile"}
    for c in F:
        if c.window == "one":
            assert c.n_out == 1
        elif c.window == "head":
            assert c.n0 == 0 and c.n_out < c.n_bins + c.T - 1
        elif c.window == "tail":
            assert c.n0 > 0 and c.n0 + c.n_out == c.n_bins + c.T - 1
        elif c.window == "tile":
            assert c.n0 < TILE < c.n0 + c.n_out
    assert any(c.gap > 0 and c.add is None for c in F) and any(c.gap > 0 and c.add for c in F)
    assert {c.add for c in F} == {None, "normal", "zeros", "nan"}
    z = inputs(by["add-zeros"])["out0"]
    assert not z.any() and np.signbit(z).any() and not np.signbit(z).all()
    assert np.isnan(inputs(by["add-nan"])["out0"]).any() and np.isnan(reference(by["add-nan"])[..., 0]).all()


@pytest.mark.parametrize("case", [c for c in CASES if c.add is None], ids=lambda c: c.id)
def test_the_gap_keeps_the_sentinel_and_a_window_is_that_window_of_the_whole(case):
    y = reference(case)
    assert (y[..., case.n_out:].view(np.uint64) == np.uint64(SENTINEL)).all()
    w = whole(case)
    assert canonical(y[..., :case.n_out]).tobytes() == canonical(w[..., case.n0:case.n0 + case.n_out]).tobytes()


@pytest.mark.parametrize("case", [c for c in CASES if c.add is not None], ids=lambda c: c.id)
def test_add_is_one_add_onto_the_rows(case):
    y, x = reference(case), inputs(case)
    w = whole(case)[..., case.n0:case.n0 + case.n_out]
    with np.errstate(all="ignore"):
        assert canonical(y[..., :case.n_out]).tobytes() == canonical(x["out0"][..., :case.n_out] + w).tobytes()
    assert y[..., case.n_out:].tobytes() == x["out0"][..., case.n_out:].tobytes()


@pytest.mark.parametrize("case", [c for c in CASES if c.K > 1 and c.add is None and c.index % 3 == 0], ids=lambda c: c.id)
def test_a_receiver_alone_is_that_receiver_of_the_call(case):
    x = inputs(case)
    for k in range(min(case.K, 3)):
        y = impulse_ref(x["hist"][k:k + 1], x["taps"], case.frac_bits, case.n0, case.n_out, x["weight"])
        assert canonical(y[0]).tobytes() == canonical(reference(case)[k, :, :case.n_out]).tobytes()


@pytest.mark.parametrize("case", [c for c in FIXED if c.name.startswith("one-") and c.name != "one-chunk-of-tile-1"], ids=lambda c: c.id)
def test_a_single_entry_gives_exactly_gain_times_tap(case):
    x = inputs(case)
    (i, b), = case.positions()
    gain, there = gains(x["hist"], case.frac_bits)
    assert there.sum() == case.K and there[0, i, b]
    y = whole(case)
    want = np.zeros_like(y)
    want[0, :, i:i + case.T] = gain[0, i, b, :, None] * x["taps"][b][None, :]          # 0.0 + x is x (and +0.0 for x = -0.0, which no product here is)
    assert y.tobytes() == want.tobytes()
    assert gain[0, i, b, 0] == np.sqrt(np.ldexp(float(x["hist"][0, i, b, 0]), -case.frac_bits))


def test_two_paths_in_one_sample_and_band_add_as_energies():
    hist = np.zeros((1, 10, 1, 1), np.uint64)
    e1, e2 = 9 << 24, 16 << 24
    hist[0, 4, 0, 0] = e1 + e2
    y = impulse_ref(hist, np.ones((1, 1)), 24)
    assert y[0, 0, 4] == 5.0 and np.count_nonzero(y) == 1


def reach(case):
    """cnt int [K, B, n_out]: the entries of band b whose taps reach output n of the case's window"""
    x = inputs(case)
    there = entries(x["hist"], x["weight"]) != 0
    cs = np.concatenate([np.zeros((case.K, 1, case.B), np.int64), np.cumsum(there, axis=1)], axis=1)          # cs[i] = entries in bins < i
    n = np.arange(case.n0, case.n0 + case.n_out)
    lo, hi = np.maximum(0, n - (case.T - 1)), np.minimum(case.n_bins - 1, n)
    return (cs[:, np.maximum(hi + 1, lo)] - cs[:, lo]).transpose(0, 2, 1)


PLAIN = [c for c in CASES if c.words == "normal" and c.taps == "normal" and c.frac_bits <= 40 and c.add is None]


def test_the_bands_descending_differ_wherever_the_sums_could_show_it():
    """Two terms commute: an output shows the order of the bands when it has three terms or more from two bands or more"""
    seen = 0
    for case in PLAIN:
        cnt = reach(case)
        if ((cnt.sum(axis=1) >= 3) & ((cnt > 0).sum(axis=1) >= 2)).sum() * case.C < 64:          # a few sums may all round alike by chance
            continue
        seen += 1
        x = inputs(case)
        y = impulse_ref(x["hist"], x["taps"], case.frac_bits, case.n0, case.n_out, x["weight"], bands="descending")
        assert y.tobytes() != reference(case)[..., :case.n_out].tobytes(), case.id
        assert np.allclose(y, reference(case)[..., :case.n_out], rtol=1e-9, atol=1e-9 * np.abs(y).max())
    assert seen >= 20


def test_the_bins_descending_differ_wherever_the_sums_could_show_it():
    """An output shows the order of the bins when one band has three terms or more in it, or two behind a term of an earlier band"""
    seen = 0
    for case in PLAIN:
        cnt = reach(case)
        before = np.cumsum(cnt, axis=1) - cnt
        if ((cnt >= 3) | ((cnt >= 2) & (before > 0))).any(axis=1).sum() * case.C < 64:          # a few sums may all round alike by chance
            continue
        seen += 1
        x = inputs(case)
        y = impulse_ref(x["hist"], x["taps"], case.frac_bits, case.n0, case.n_out, x["weight"], bins="descending")
        assert y.tobytes() != reference(case)[..., :case.n_out].tobytes(), case.id
        assert np.allclose(y, reference(case)[..., :case.n_out], rtol=1e-9, atol=1e-9 * np.abs(y).max())
    assert seen >= 20


def test_the_order_cases_are_among_them():
    by = {c.name: c for c in FIXED}
    cnt = reach(by["three-one-band"])
    assert (cnt >= 3).any()
    cnt = reach(by["three-two-bands"])
    assert ((cnt.sum(axis=1) >= 3) & ((cnt > 0).sum(axis=1) >= 2)).any()
    assert by["three-one-band"] in PLAIN and by["three-two-bands"] in PLAIN
