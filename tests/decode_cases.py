"""The cases of the tests of the decoding (tests/test_decode_cases.py on the reference alone, tests/test_gpu_decode.py on the device), in the
manner of tests/convolve_cases.py: a case type, a list that covers shapes, windows and value classes pairwise rather than as a full
product, inputs from a seed, and the reference (tests/decode_ref.py) computed once per case.  The kernel's tile is the convolution's
(hare_amd/csrc/hare_device.h: kDecode* = kConvolve*), so the tile, the tap chunk and the tap block come from tests/convolve_cases.py, and
the windows and the placements of the lone infinity and NaN are put at their edges.  At most 200 cases, each under 2^24 terms.
No GPU, no torch."""
import re
from functools import lru_cache

import numpy as np

from tests.convolve_cases import _DEVICE_H, BLOCK, CHUNK, LDS_BYTES, THREADS, TILE
from tests.decode_ref import decode_ref

for _n in ("Threads", "Run", "Tile", "Chunk", "Block", "LdsDoubles"):          # the decode launch IS the convolution's
    assert re.search(r"constexpr int kDecode%s = kConvolve%s;" % (_n, _n), _DEVICE_H), _n

MAX_TERMS = 1 << 24


def plan(K, O, n_out):
    """decode_plan's launch: (grid, block, dynamic LDS bytes)"""
    return K * O * -(-n_out // TILE), THREADS, LDS_BYTES


N_LIST = [1, 2, 63, 64, 65, 543, 544, 2048, 2049, 4097]
T_LIST = [1, 2, 31, 32, 33, 64, 255, 256, 257, 600]
C_LIST = [1, 3, 4, 9, 16]
O_LIST = [1, 2, 5]
K_LIST = [1, 3]
WINDOWS = ("whole", "one", "tile-+", "tile+-", "last", "head", "tail", "middle")
VALUES = ("normal", "zeros", "huge")
SPECIALS = tuple(f"{what}:{arr}:{where}:{ch}" for what in ("inf", "nan") for arr in ("in", "h") for where in ("first", "last", "chunk")
                 for ch in ("c0", "cl"))

# Seeds.  A case draws from SEED + index.  With this SEED each of the three wrong orders of tests/decode_ref.py differs from the definition
# on every case that could show it (a window of one output need not, by chance): tests/test_decode_cases.py checks that on every run, and
# a change of the list that breaks it takes another SEED.
SEED = 7000


class Case:
    """window: "whole"; "one" (the middle sample alone); "tile-+" / "tile+-" (from one sample before / behind the whole call's first tile
    edge to one sample behind / before its second); "last" (the last sample alone); "head" (every output with t_lo = 0 and t_hi < T - 1);
    "tail" (every output with t_lo > 0 and t_hi = T - 1); "middle" (every output whose
    range has min(N, T) taps).  values: "normal" (standard normals); "zeros" (signed zeros and denormals among normals); "huge"
    (magnitudes near 2^500 and 2^-500: products overflow and underflow); or "<inf|nan>:<in|h>:<where>:<c0|cl>", normals with ONE
    infinity or NaN in `in` or `h`, in the first channel or the last, at index 0 ("first"), at the last index ("last") or at the
    tap-chunk edge ("chunk")."""

    def __init__(self, index, K, C, N, O, T, window="whole", values="normal"):
        self.index, self.K, self.C, self.N, self.O, self.T, self.window, self.values = index, K, C, N, O, T, window, values
        self.id = f"{index}-K{K}-C{C}-N{N}-O{O}-T{T}-{window}-{values}"
        total = N + T - 1
        lo, hi = min(N, T), max(N, T)
        self.n0, self.n_out = {
            "whole": (0, total), "one": (total // 2, 1), "tile-+": (TILE - 1, TILE + 2), "tile+-": (TILE + 1, TILE - 2), "last": (total - 1, 1),
            "head": (0, min(N, T - 1)), "tail": (max(T - 1, N), total - max(T - 1, N)), "middle": (lo - 1, hi - lo + 1)}[window]
        assert self.n0 >= 0 and self.n_out >= 1 and self.n0 + self.n_out <= total, self.id

    @property
    def terms(self):
        """the call's bound: K x O x n_out x C x min(N, T)"""
        return self.K * self.O * self.n_out * self.C * min(self.N, self.T)

    @property
    def middle_terms(self):
        """the terms of the sum of the window's middle output"""
        n = self.n0 + self.n_out // 2
        return self.C * (min(self.T - 1, n) - max(0, n - (self.N - 1)) + 1)


def special_index(case):
    """(array name, channel, index within the row of `in` or the filter of `h`) of the lone value of a special case"""
    _, arr, where, ch = case.values.split(":")
    n = case.N if arr == "in" else case.T
    return arr, 0 if ch == "c0" else case.C - 1, {"first": 0, "last": n - 1, "chunk": CHUNK if n > CHUNK else n // 2}[where]


@lru_cache(maxsize=None)
def inputs(case):
    """(in float64 [K, C, N], h float64 [O, C, T]), read-only"""
    rng = np.random.default_rng(SEED + case.index)
    x, h = rng.standard_normal((case.K, case.C, case.N)), rng.standard_normal((case.O, case.C, case.T))
    if case.values == "zeros":
        for a in (x, h):
            kind = rng.integers(0, 4, a.shape)
            tiny = rng.integers(1, 1 << 50, a.shape).astype(np.float64) * 5e-324 * rng.choice([-1.0, 1.0], a.shape)
            a[kind == 0] = 0.0
            a[kind == 1] = -0.0
            a[kind == 2] = tiny[kind == 2]
    elif case.values == "huge":
        for a in (x, h):
            a[...] = np.ldexp(rng.uniform(1.0, 2.0, a.shape), rng.choice([-500, 500], a.shape)) * rng.choice([-1.0, 1.0], a.shape)
    elif ":" in case.values:
        arr, c, at = special_index(case)
        v = np.inf if case.values.startswith("inf") else np.nan
        if arr == "in":
            x[case.K // 2, c, at] = v
        else:
            h[case.O // 2, c, at] = v
    x.flags.writeable = False
    h.flags.writeable = False
    return x, h


@lru_cache(maxsize=None)
def reference(case):
    x, h = inputs(case)
    y = decode_ref(x, h, case.n0, case.n_out)
    y.flags.writeable = False
    return y


def _cases():
    c = []

    def add(K, C, N, O, T, window="whole", values="normal", keep=()):
        """the case, made smaller until it is under MAX_TERMS: K first, then O, then C -- never a dimension named in `keep`"""
        while True:
            case = Case(len(c), K, C, N, O, T, window, values)
            if case.terms < MAX_TERMS:
                break
            if K > 1 and "K" not in keep:
                K = 1
            elif O > 1 and "O" not in keep:
                O = O_LIST[O_LIST.index(O) - 1]
            elif C > 1 and "C" not in keep:
                C = C_LIST[C_LIST.index(C) - 1]
            else:
                raise AssertionError(case.id)
        c.append(case)

    # every N with every T, the whole output; C, O, K and the plain value classes go round
    for i, N in enumerate(N_LIST):
        for j, T in enumerate(T_LIST):
            add(K_LIST[(i + j // 2) % 2], C_LIST[(i + j) % 5], N, O_LIST[(i + 2 * j) % 3], T, "whole", VALUES[(i + j // 3) % 3])
    # every window on shapes with N > T (interior blocks, and the edge path alone), N < T and N = T; "last" never on plain normals
    shapes = [(4097, 600), (4097, 33), (2049, 257), (543, 2), (65, 600), (2, 257), (256, 256)]
    for s, (N, T) in enumerate(shapes):
        for w, window in enumerate(WINDOWS):
            if window.startswith("tile") and N + T - 1 < 2 * TILE + 1:
                continue
            values = VALUES[(s + w) % 3]
            if window == "last" and values == "normal":
                values = "zeros"
            add(K_LIST[(s + w) % 2], C_LIST[(s + 2 * w) % 5], N, O_LIST[(s + w) % 3], T, window, values)
    # the lone infinity and the lone NaN: every placement on a shape with N > T, every second one on a shape with N < T and, around the
    # tile edges, on one of more than two tiles; the windows going round
    for v, values in enumerate(SPECIALS):
        add(K_LIST[v % 2], 3, 2049, O_LIST[v % 3], 600, ("whole", "last", "head", "tail", "one", "middle")[v % 6], values)
    for v, values in enumerate(SPECIALS):
        if (v + v // 2) % 2 == 0:
            add(K_LIST[v % 2], 4, 257, 2, 600, ("whole", "tail", "head", "one", "last")[(v // 2) % 5], values)
        else:
            add(3, 4, 4097, 2, 257, ("tile-+", "tile+-", "whole")[(v // 2) % 3], values)
    # the pairs of a shape with a channel count that the lists above left out (a large shape is made smaller in C and O there): the other
    # length short
    for name, LIST in (("C", C_LIST), ("O", O_LIST)):
        for N in N_LIST:
            for v in LIST:
                if not any(k.N == N and getattr(k, name) == v for k in c):
                    add(1, v if name == "C" else 3, N, v if name == "O" else 2, 33, "whole", VALUES[len(c) % 3], keep=(name,))
        for T in T_LIST:
            for v in LIST:
                if not any(k.T == T and getattr(k, name) == v for k in c):
                    add(1, v if name == "C" else 3, 65, v if name == "O" else 2, T, "whole", VALUES[len(c) % 3], keep=(name,))
    # plain normals through the interior path at every C and O, and K = 3 on a window of more than one tile
    for C in C_LIST:
        add(1, C, 1000, O_LIST[C % 3], 96, "whole", "normal", keep=("C",))
    add(3, 4, 4097, 2, 96, "tile-+", "normal", keep=("K", "C", "O"))
    return c


CASES = _cases()
assert len(CASES) <= 200, len(CASES)
