"""The convolution's cases and its restatement (tests/convolve_cases.py, tests/convolve_ref.py) without a GPU: every class the device test
is to meet is in the list; the references are pinned by digest (tests/golden/convolve_reference_digests.json, NaNs canonicalised); a window
of the reference is that window of the whole; a lone infinity reaches exactly the outputs whose range holds it; and on every plain-normal
case with min(N, L) >= 8 the mutant that sums in descending t differs from the definition in at least one output word -- so a device that
walked the taps the wrong way round could not pass tests/test_gpu_convolve.py."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests.convolve_cases import BLOCK, CASES, CHUNK, L_LIST, N_LIST, R_LIST, SPECIALS, TILE, VALUES, WINDOWS, inputs, plan, reference, special_index
from tests.convolve_ref import canonical, convolve_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convolve_reference_digests.json")


def digest(y):
    return hashlib.sha256(np.ascontiguousarray(canonical(y)).tobytes()).hexdigest()


def test_the_list_follows_the_kernels_plan():
    assert (TILE, CHUNK, BLOCK) == (2048, 256, 32) and TILE % CHUNK == 0 and CHUNK % BLOCK == 0
    assert {CHUNK - 1, CHUNK + 1} <= set(N_LIST)
    assert plan(3, TILE) == (3, 256, 8 * (256 + 9 * 288)) and plan(3, TILE + 1)[0] == 6


def test_every_class_named_is_in_the_list():
    assert {c.N for c in CASES} >= set(N_LIST) >= {1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097}
    assert {c.L for c in CASES} >= set(L_LIST) == {1, 2, 64, 257, 1000, 5000}
    assert {c.R for c in CASES} == set(R_LIST) == {1, 3, 16, 67}
    assert {(c.N, c.L) for c in CASES} >= {(N, L) for N in N_LIST for L in L_LIST}
    assert {c.window for c in CASES} == set(WINDOWS)
    assert {c.values for c in CASES} == set(VALUES) | set(SPECIALS)
    for window in WINDOWS:
        if window != "middle":
            assert {c.N > c.L for c in CASES if c.window == window} == {True, False}, window
    assert all(c.N > c.L for c in CASES if c.window == "middle")
    for values in VALUES:
        assert {c.N > c.L for c in CASES if c.values == values} == {True, False}, values
    # every pair of R with a window kind and with a plain value class
    assert {(c.R, c.values) for c in CASES} >= {(R, v) for R in R_LIST for v in VALUES}
    assert len({c.id for c in CASES}) == len(CASES) and max(c.terms for c in CASES) <= 16 * 9096 * 4097
    assert any(c.n_out > TILE and c.R == 67 for c in CASES)


@pytest.mark.parametrize("case", [c for c in CASES if c.window != "whole"], ids=lambda c: c.id)
def test_a_window_holds_what_it_names(case):
    N, L, n = case.N, case.L, np.arange(case.n0, case.n0 + case.n_out)
    t_lo, t_hi = np.maximum(0, n - (L - 1)), np.minimum(N - 1, n)
    w = case.window
    if w in ("one", "last"):
        assert case.n_out == 1 and (w == "one" or n[0] == N + L - 2)
        assert w == "last" or t_hi[0] - t_lo[0] + 1 >= min(N, L) - 1
    elif w == "head":
        nxt = n[-1] + 1                                                  # the first output behind the head is not of it
        assert (t_lo == 0).all() and (t_hi < N - 1).all() and n[0] == 0 and (nxt > L - 1 or nxt >= N - 1)
    elif w == "tail":
        prev = n[0] - 1                                                  # the last output before the tail is not of it
        assert (t_lo > 0).all() and (t_hi == N - 1).all() and n[-1] == N + L - 2 and (prev <= L - 1 or prev < N - 1)
    elif w == "middle":
        assert (t_hi - t_lo + 1 == L).all() and (n[0] == L - 1) and n[-1] == N - 1
    else:
        assert (n[0], n[-1]) == {"tile-+": (TILE - 1, 2 * TILE), "tile+-": (TILE + 1, 2 * TILE - 2)}[w]


def test_a_window_of_the_reference_is_that_window_of_the_whole():
    for case in CASES:
        if case.window == "whole" or case.R * (case.N + case.L - 1) * min(case.N, case.L) > 1 << 28:
            continue
        ir, x = inputs(case)
        whole = convolve_ref(ir, x)
        assert canonical(whole[:, case.n0:case.n0 + case.n_out]).tobytes() == canonical(reference(case)).tobytes(), case.id


@pytest.mark.parametrize("case", [c for c in CASES if c.values.startswith("inf") and c.window == "whole"], ids=lambda c: c.id)
def test_a_lone_infinity_reaches_exactly_the_outputs_whose_range_holds_it(case):
    """Every other value is a normal, so nothing turns the infinity into a NaN: a reference (or a device) that formed out-of-range terms
    against zeros would show NaNs"""
    arr, at = special_index(case)
    y = reference(case)
    n = np.arange(case.n_out)
    if arr == "ir":
        hit = np.zeros(y.shape, bool)
        hit[case.R // 2] = (n >= at) & (n <= at + case.L - 1)
    else:
        hit = np.broadcast_to((n >= at) & (n <= at + case.N - 1), y.shape)
    assert np.array_equal(np.isinf(y), hit) and not np.isnan(y).any()


def test_the_accumulator_is_never_minus_zero():
    for case in CASES:
        y = reference(case)
        assert not (np.signbit(y) & (y == 0)).any(), case.id


MUTABLE = [c for c in CASES if c.values == "normal" and min(c.N, c.L) >= 8]


def test_a_descending_sum_is_seen_on_every_plain_normal_case():
    assert len(MUTABLE) >= 20
    for case in MUTABLE:
        ir, x = inputs(case)
        mutant = convolve_ref(ir, x, case.n0, case.n_out, descending=True)
        assert np.isfinite(mutant).all()
        assert (mutant.view(np.uint64) != reference(case).view(np.uint64)).any(), case.id


def test_the_order_cases_depend_on_the_order():
    order = [c for c in CASES if c.values == "order" and min(c.N, c.L) >= 8 and c.n_out > 1]
    assert len(order) >= 5
    for case in order:
        ir, x = inputs(case)
        assert set(np.abs(ir).ravel().tolist()) == {1.0, 2.0 ** 52}
        assert (convolve_ref(ir, x, case.n0, case.n_out, descending=True) != reference(case)).any(), case.id


def test_references_are_pinned_by_digest():
    want = json.load(open(GOLDEN))
    got = {c.id: digest(reference(c)) for c in CASES}
    assert sorted(got) == sorted(want)
    assert [k for k in got if got[k] != want[k]] == []
