"""The decoding's cases and its restatement (tests/decode_cases.py, tests/decode_ref.py) without a GPU: the list covers its shapes pairwise
under its two caps; every case holds the class it names; the references are pinned by digest (tests/golden/decode_reference_digests.json,
NaNs canonicalised); a window of the reference is that window of the whole; a lone infinity reaches exactly the outputs whose range holds
it; with C = O = 1 the restatement is the convolution's on the convolution's own cases, byte for byte; and each of three wrong orders --
the channels descending, t outside and c inside, per-channel convolutions added afterwards (what hare_convolve per channel and a host add
would give) -- differs from the definition on every plain-normal case that could show it, so a device that summed in one of them could
not pass tests/test_gpu_decode.py."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import convolve_cases
from tests.convolve_ref import canonical
from tests.decode_cases import (BLOCK, C_LIST, CASES, CHUNK, K_LIST, MAX_TERMS, N_LIST, O_LIST, SPECIALS, T_LIST, TILE, VALUES, WINDOWS, inputs, plan,
                                reference, special_index)
from tests.decode_ref import ORDERS, decode_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_reference_digests.json")


def digest(y):
    return hashlib.sha256(np.ascontiguousarray(canonical(y)).tobytes()).hexdigest()


def test_the_list_follows_the_kernels_plan():
    assert (TILE, CHUNK, BLOCK) == (2048, 256, 32)
    assert {CHUNK - 1, CHUNK, CHUNK + 1, BLOCK - 1, BLOCK, BLOCK + 1} <= set(T_LIST) and {TILE, TILE + 1, 2 * TILE + 1} <= set(N_LIST)
    assert {64 * 8 + BLOCK - 1, 64 * 8 + BLOCK} <= set(N_LIST)          # the shortest input whose wave has an interior block of 32 taps, and one less
    assert plan(3, 2, TILE) == (6, 256, 8 * (256 + 9 * 288)) and plan(3, 2, TILE + 1)[0] == 12


def test_the_list_is_a_pairwise_cover_under_its_caps():
    assert len(CASES) <= 200 and len({c.id for c in CASES}) == len(CASES)
    assert max(c.terms for c in CASES) < MAX_TERMS == 1 << 24
    assert N_LIST == [1, 2, 63, 64, 65, 543, 544, 2048, 2049, 4097] and T_LIST == [1, 2, 31, 32, 33, 64, 255, 256, 257, 600]
    assert (C_LIST, O_LIST, K_LIST) == ([1, 3, 4, 9, 16], [1, 2, 5], [1, 3])
    lists = dict(N=N_LIST, T=T_LIST, C=C_LIST, O=O_LIST, K=K_LIST)
    for a in lists:
        for b in lists:
            if a < b:
                have = {(getattr(c, a), getattr(c, b)) for c in CASES}
                assert have >= {(x, y) for x in lists[a] for y in lists[b]}, (a, b)
    assert {c.window for c in CASES} == set(WINDOWS)
    assert {c.values for c in CASES} == set(VALUES) | set(SPECIALS) and len(SPECIALS) == 24
    for window in WINDOWS:          # two tiles and a sample take N > T: no T of the list is that long
        assert {c.N > c.T for c in CASES if c.window == window} == ({True} if window.startswith("tile") else {True, False}), window
    for values in VALUES:
        assert {c.N > c.T for c in CASES if c.values == values} == {True, False}, values
        assert {c.C for c in CASES if c.values == values} == set(C_LIST), values
    assert any(c.n_out > TILE and c.K == 3 and c.O > 1 and c.C > 1 for c in CASES)


@pytest.mark.parametrize("case", [c for c in CASES if c.window != "whole"], ids=lambda c: c.id)
def test_a_window_holds_what_it_names(case):
    N, T, n = case.N, case.T, np.arange(case.n0, case.n0 + case.n_out)
    t_lo, t_hi = np.maximum(0, n - (N - 1)), np.minimum(T - 1, n)
    w = case.window
    if w in ("one", "last"):
        assert case.n_out == 1 and (w == "one" or n[0] == N + T - 2)
        assert w == "last" or t_hi[0] - t_lo[0] + 1 >= min(N, T) - 1
    elif w == "head":
        nxt = n[-1] + 1                                                  # the first output behind the head is not of it
        assert (t_lo == 0).all() and (t_hi < T - 1).all() and n[0] == 0 and (nxt > N - 1 or nxt >= T - 1)
    elif w == "tail":
        prev = n[0] - 1                                                  # the last output before the tail is not of it
        assert (t_lo > 0).all() and (t_hi == T - 1).all() and n[-1] == N + T - 2 and (prev <= N - 1 or prev < T - 1)
    elif w == "middle":
        assert (t_hi - t_lo + 1 == min(N, T)).all() and n[0] == min(N, T) - 1 and n[-1] == max(N, T) - 1
    else:
        assert (n[0], n[-1]) == {"tile-+": (TILE - 1, 2 * TILE), "tile+-": (TILE + 1, 2 * TILE - 2)}[w]


@pytest.mark.parametrize("values", VALUES + ("special",))
def test_the_values_hold_the_class_they_name(values):
    mine = [c for c in CASES if (c.values == values if values != "special" else ":" in c.values)]
    assert mine
    for case in mine:
        x, h = inputs(case)
        assert x.shape == (case.K, case.C, case.N) and h.shape == (case.O, case.C, case.T) and x.dtype == h.dtype == np.float64
        both = np.concatenate([x.ravel(), h.ravel()])
        if values == "normal":
            assert np.isfinite(both).all() and (both != 0).all() and (np.abs(both) < 8).all()
        elif values == "zeros":
            tiny = (both != 0) & (np.abs(both) < 2.0 ** -1022)
            assert np.isfinite(both).all()
            if both.size >= 64:
                assert ((both == 0) & ~np.signbit(both)).any() and ((both == 0) & np.signbit(both)).any() and tiny.any() and (np.abs(both) > 1e-3).any()
        elif values == "huge":
            e = np.frexp(both)[1]
            assert np.isfinite(both).all() and set(np.unique(e)) <= {-499, 501}
            if both.size >= 64:
                assert set(np.unique(e)) == {-499, 501} and (both < 0).any() and (both > 0).any()
        else:
            what, arr, where, ch = case.values.split(":")
            name, c, at = special_index(case)
            a, other = (x, h) if arr == "in" else (h, x)
            assert name == arr and c == (0 if ch == "c0" else case.C - 1) and case.C > 1 and np.isfinite(other).all()
            bad = np.argwhere(~np.isfinite(a))
            assert bad.tolist() == [[(case.K if arr == "in" else case.O) // 2, c, at]], case.id
            assert (np.isinf if what == "inf" else np.isnan)(a[tuple(bad[0])])
            n = a.shape[2]
            assert at == {"first": 0, "last": n - 1, "chunk": CHUNK}[where] and n > CHUNK


def test_a_window_of_the_reference_is_that_window_of_the_whole():
    seen = 0
    for case in CASES:
        if case.window == "whole" or case.K * case.O * (case.N + case.T - 1) * case.C * min(case.N, case.T) >= 4 * MAX_TERMS:
            continue
        x, h = inputs(case)
        whole = decode_ref(x, h)
        assert canonical(whole[:, :, case.n0:case.n0 + case.n_out]).tobytes() == canonical(reference(case)).tobytes(), case.id
        seen += 1
    assert seen >= 40


@pytest.mark.parametrize("case", [c for c in CASES if c.values.startswith("inf")], ids=lambda c: c.id)
def test_a_lone_infinity_reaches_exactly_the_outputs_whose_range_holds_it(case):
    """Every other value is a normal and the infinity meets every output in at most one term, so nothing turns it into a NaN: a reference
    (or a device) that formed out-of-range terms against zeros would show NaNs"""
    arr, _, at = special_index(case)
    y = reference(case)
    n = np.arange(case.n0, case.n0 + case.n_out)
    hit = np.zeros(y.shape, bool)
    if arr == "in":
        hit[case.K // 2, :] = (n >= at) & (n <= at + case.T - 1)
    else:
        hit[:, case.O // 2] = (n >= at) & (n <= at + case.N - 1)
    assert np.array_equal(np.isinf(y), hit) and not np.isnan(y).any()


def test_the_accumulator_is_never_minus_zero():
    for case in CASES:
        y = reference(case)
        assert not (np.signbit(y) & (y == 0)).any(), case.id


def test_one_channel_and_one_output_is_the_convolution_byte_for_byte():
    """hare_convolve with ir = h (its N this T) and x = in[k] (its L this N): the header says so of the calls, this of the restatements, on
    the convolution's own cases of one row"""
    mine = [c for c in convolve_cases.CASES if c.R == 1]
    assert len(mine) >= 20 and {c.window for c in mine} == set(convolve_cases.WINDOWS)
    for case in mine:
        ir, x = convolve_cases.inputs(case)
        y = decode_ref(x[None, None, :], ir[None, :, :], case.n0, case.n_out)
        assert y.shape == (1, 1, case.n_out)
        assert canonical(y[0]).tobytes() == canonical(convolve_cases.reference(case)).tobytes(), case.id


MUTABLE = [c for c in CASES if c.values == "normal" and c.C >= 2 and c.T >= 2 and c.middle_terms >= 64]


@pytest.mark.parametrize("order", ORDERS[1:])
def test_a_wrong_order_is_seen_on_every_plain_normal_case(order):
    assert len(MUTABLE) >= 20 and {c.window for c in MUTABLE} >= {"whole", "one", "head", "tail", "middle"} and any(c.window.startswith("tile") for c in MUTABLE)
    for case in MUTABLE:
        x, h = inputs(case)
        mutant = decode_ref(x, h, case.n0, case.n_out, order)
        assert np.isfinite(mutant).all()
        assert (mutant.view(np.uint64) != reference(case).view(np.uint64)).any(), case.id


def test_references_are_pinned_by_digest():
    want = json.load(open(GOLDEN))
    got = {c.id: digest(reference(c)) for c in CASES}
    assert sorted(got) == sorted(want)
    assert [k for k in got if got[k] != want[k]] == []
