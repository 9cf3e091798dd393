"""The cases of the tests of the convolution (tests/test_convolve_cases.py on the reference alone, tests/test_gpu_convolve.py on the device):
a case type, a list that covers shapes, windows and value classes pairwise rather than as a full product, inputs from a seed, and the
reference (tests/convolve_ref.py) computed once per case.  The list follows the kernel: the output tile, the tap chunk and the tap block
are read from hare_amd/csrc/hare_device.h (what convolve_plan, hist.cpp, launches with), and the windows and the placements of the lone
infinity and NaN are put at their edges.  The largest reference is 16 x 9 096 x 4 097 terms; the whole list takes well under a minute.
No GPU, no torch."""
import os
import re
from functools import lru_cache

import numpy as np

from tests.convolve_ref import convolve_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DEVICE_H = open(os.path.join(ROOT, "hare_amd", "csrc", "hare_device.h")).read()


def _const(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, _DEVICE_H).group(1))


THREADS, RUN, TILE, CHUNK, BLOCK = (_const("kConvolve" + n) for n in ("Threads", "Run", "Tile", "Chunk", "Block"))
LDS_BYTES = 8 * (CHUNK + 9 * ((TILE + CHUNK + 7) // 8))          # kConvolveLdsDoubles, restated
assert TILE == THREADS * RUN


def plan(R, n_out):
    """convolve_plan's launch: (grid, block, dynamic LDS bytes)"""
    return R * -(-n_out // TILE), THREADS, LDS_BYTES


N_LIST = sorted({1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, CHUNK - 1, CHUNK + 1})
L_LIST = [1, 2, 64, 257, 1000, 5000]
R_LIST = [1, 3, 16, 67]
WINDOWS = ("whole", "one", "tile-+", "tile+-", "last", "head", "tail", "middle")
VALUES = ("normal", "zeros", "huge", "order")
SPECIALS = tuple(f"{what}:{arr}:{where}" for what in ("inf", "nan") for arr in ("ir", "x") for where in ("first", "last", "chunk"))


class Case:
    """window: "whole"; "one" (the middle sample alone); "tile-+" / "tile+-" (from one sample before / behind the whole call's first tile
    edge to one sample behind / before its second); "last" (the last sample alone); "head" (every output with t_lo = 0 and t_hi < N - 1);
    "tail" (every output with t_lo > 0 and t_hi = N - 1); "middle" (N > L: every output that meets all of x).  values: "normal" (standard
    normals); "zeros" (signed zeros and denormals among normals); "huge" (magnitudes near 2^500 and 2^-500: products overflow and
    underflow); "order" (ir alternates +2^52, 1.0, -2^52, 1.0: the order of the sum decides the result); or "<inf|nan>:<ir|x>:<where>", normals
    with ONE infinity or NaN in ir or x at index 0 ("first"), at the last index ("last") or at the tap-chunk edge ("chunk")."""

    def __init__(self, index, R, N, L, window="whole", values="normal"):
        self.index, self.R, self.N, self.L, self.window, self.values = index, R, N, L, window, values
        self.id = f"{index}-R{R}-N{N}-L{L}-{window}-{values}"
        total = N + L - 1
        self.n0, self.n_out = {
            "whole": (0, total), "one": (total // 2, 1), "tile-+": (TILE - 1, TILE + 2), "tile+-": (TILE + 1, TILE - 2), "last": (total - 1, 1),
            "head": (0, min(L, N - 1)), "tail": (max(N - 1, L), total - max(N - 1, L)), "middle": (L - 1, N - L + 1)}[window]
        assert self.n0 >= 0 and self.n_out >= 1 and self.n0 + self.n_out <= total, self.id

    @property
    def terms(self):
        return self.R * self.n_out * min(self.N, self.L)


def special_index(case):
    """(array name, flat index within a row or x) of the lone value of a special case"""
    _, arr, where = case.values.split(":")
    n = case.N if arr == "ir" else case.L
    return arr, {"first": 0, "last": n - 1, "chunk": CHUNK if n > CHUNK else n // 2}[where]


@lru_cache(maxsize=None)
def inputs(case):
    """(ir float64 [R, N], x float64 [L]), read-only"""
    rng = np.random.default_rng(9000 + case.index)
    R, N, L = case.R, case.N, case.L
    ir, x = rng.standard_normal((R, N)), rng.standard_normal(L)
    if case.values == "zeros":
        for a in (ir, x):
            kind = rng.integers(0, 4, a.shape)
            tiny = rng.integers(1, 1 << 50, a.shape).astype(np.float64) * 5e-324 * rng.choice([-1.0, 1.0], a.shape)
            a[kind == 0] = 0.0
            a[kind == 1] = -0.0
            a[kind == 2] = tiny[kind == 2]
    elif case.values == "huge":
        for a in (ir, x):
            a[...] = np.ldexp(rng.uniform(1.0, 2.0, a.shape), rng.choice([-500, 500], a.shape)) * rng.choice([-1.0, 1.0], a.shape)
    elif case.values == "order":
        ir[...] = np.array([2.0 ** 52, 1.0, -2.0 ** 52, 1.0])[np.arange(N) % 4][None, :]
        x[...] = rng.choice([1.0, 1.5, 0.5, 3.0], L)
    elif ":" in case.values:
        arr, at = special_index(case)
        v = np.inf if case.values.startswith("inf") else np.nan
        if arr == "ir":
            ir[R // 2, at] = v
        else:
            x[at] = v
    ir.flags.writeable = False
    x.flags.writeable = False
    return ir, x


@lru_cache(maxsize=None)
def reference(case):
    ir, x = inputs(case)
    y = convolve_ref(ir, x, case.n0, case.n_out)
    y.flags.writeable = False
    return y


def _cases():
    c = []

    def add(R, N, L, window="whole", values="normal"):
        case = Case(len(c), R, N, L, window, values)
        while R > 1 and case.terms > 16 * 9096 * 4097:                         # the largest reference: 16 x 9 096 x 4 097 terms
            R = R_LIST[R_LIST.index(R) - 1]
            case = Case(len(c), R, N, L, window, values)
        c.append(case)

    # every N with every L, the whole output; R and the plain value classes go round
    k = 0
    for N in N_LIST:
        for L in L_LIST:
            add(R_LIST[k % 4], N, L, "whole", VALUES[(k // 4 + k) % 4])
            k += 1
    # every window on shapes with N > L, N < L and N = L; "last" never on plain normals (one term: no order to see)
    shapes = [(4097, 1000), (4097, 64), (1000, 257), (CHUNK + 1, 2), (1000, 5000), (257, 1000), (64, 5000), (2, 257), (1000, 1000)]
    for s, (N, L) in enumerate(shapes):
        for w, window in enumerate(WINDOWS):
            if window == "middle" and N <= L:
                continue
            if window.startswith("tile") and N + L - 1 < 2 * TILE + 1:
                continue
            values = VALUES[(s + w) % 4]
            if window == "last" and values == "normal":
                values = "zeros"
            add(R_LIST[(s + w) % 4], N, L, window, values)
    # the lone infinity and the lone NaN: every placement, on a shape with N > L and one with N < L, the windows going round
    for s, (N, L) in enumerate([(1000, 257), (257, 1000), (4097, 5000)]):
        for v, values in enumerate(SPECIALS):
            window = ("whole", "last", "head", "tail", "one")[(v + s) % 5] if s < 2 else ("tile-+", "tile+-", "whole")[v % 3]
            add(R_LIST[(v + s) % 4] if s < 2 else 3, N, L, window, values)
    # plain normals through the interior path at every R, and R = 67 on a window of more than one tile
    for R in R_LIST:
        add(R, 1000, 1000, "whole", "normal")
    add(67, 4097, 5000, "tile-+", "normal")
    add(16, 4097, 5000, "whole", "normal")
    return c


CASES = _cases()
