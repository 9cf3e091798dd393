"""numpy restatement of the point source (include/hare_hip.h, "receivers", "Source"): the rays a source emits and their starting state,
operation for operation in FP64 (numpy evaluates every product, quotient and sum on its own: no contraction; its sqrt and division are
correctly rounded).  Built on tests/scatter_ref.py's RNG: the rejection step is scatter_ref.disc at counter c = 4096.  hare_emit_source's
output must match emit() bit for bit.  FRAMES, SIZES, ... are the axes of the device cases of tests/test_gpu_source.py;
tests/test_source_api.py checks on the CPU that they reach every path of the lookup."""
import numpy as np

from tests.scatter_ref import TRIES, disc, ray_base, uniform

COUNTER = 4096                      # the casts use c < 4096


def directions(seed, first_ray, n):
    """d [n, 3] of the rays first_ray .. first_ray + n - 1, and s [n] of the accepted disc point (0 with x = y = 0: none accepted)."""
    g = np.uint64(int(first_ray)) + np.arange(int(n), dtype=np.uint64)
    x, y, s = disc(ray_base(seed, g), COUNTER)
    h = np.sqrt(1.0 - s)
    return np.stack([(2.0 * x) * h, (2.0 * y) * h, 1.0 - 2.0 * s], axis=1), s


def exhausted(seed, first_ray, n):
    """The rays none of whose 32 tries fell inside the unit disc: bool [n]."""
    g = np.uint64(int(first_ray)) + np.arange(int(n), dtype=np.uint64)
    base = ray_base(seed, g)
    out = np.ones(int(n), bool)
    for t in range(TRIES):
        x = 2.0 * uniform(base, COUNTER, 1 + 2 * t) - 1.0
        y = 2.0 * uniform(base, COUNTER, 2 + 2 * t) - 1.0
        out &= ~(x * x + y * y < 1.0)
    return out


def lookup(d, frame, R):
    """The cube-map texel of every direction: (F, iv, iu) int arrays [n], and a dict of which paths the lookup took:
    faces (set of F), clamped (any tu or tv >= R), ties (set of 'a0=a1', 'a0=a2', 'a1=a2', 'all' seen among the leading axes), nan
    (any NaN tu or tv)."""
    M = np.asarray(frame, np.float64).reshape(3, 3)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    l = [(M[i, 0] * dx + M[i, 1] * dy) + M[i, 2] * dz for i in range(3)]
    a = [np.abs(v) for v in l]
    f = np.zeros(len(dx), np.int64)
    af = a[0].copy()
    m1 = a[1] > af
    f[m1] = 1
    af = np.where(m1, a[1], af)
    m2 = a[2] > af
    f[m2] = 2
    af = np.where(m2, a[2], af)
    L = np.stack(l, axis=1)
    idx = np.arange(len(dx))
    lf, lu, lv = L[idx, f], L[idx, (f + 1) % 3], L[idx, (f + 2) % 3]
    F = 2 * f + (lf < 0)
    Rd = np.float64(R)
    half = 0.5 * Rd

    def texel(lw):
        with np.errstate(invalid="ignore", divide="ignore"):
            t = (lw / af + 1.0) * half
            inside = np.floor(np.where((t >= 0) & (t < Rd), t, 0.0)).astype(np.int64)
            return np.where(t >= 0, np.where(t < Rd, inside, R - 1), 0), t
    iu, tu = texel(lu)
    iv, tv = texel(lv)
    ties = set()
    if np.any((a[0] == a[1]) & (a[0] == a[2])):
        ties.add("all")
    for i, j in ((0, 1), (0, 2), (1, 2)):
        k = 3 - i - j
        if np.any((a[i] == a[j]) & (a[i] >= a[k])):
            ties.add("a%d=a%d" % (i, j))
    with np.errstate(invalid="ignore"):
        paths = dict(faces=set(int(v) for v in np.unique(F)), clamped=bool(np.any(tu >= Rd) or np.any(tv >= Rd)), ties=ties,
                     nan=bool(np.any(tu != tu) or np.any(tv != tv)))
    return F, iv, iu, paths


def emit(seed, first_ray, n, pos, power, frame, R, gain, paths=None):
    """rays [n, 6] and state [1 + B, n] of the rays first_ray .. first_ray + n - 1: ray = (pos, d), L = 0, E[b] = power[b] * gain_b(d).
    power [B]; frame [3, 3] or None (identity); gain [6, R, R, B] or None with R = 0 (every gain 1.0).  paths (dict, optional) receives
    lookup()'s record of the paths taken."""
    n = int(n)
    power = np.asarray(power, np.float64).reshape(-1)
    B = power.shape[0]
    d, _ = directions(seed, first_ray, n)
    rays = np.empty((n, 6), np.float64)
    rays[:, :3] = np.asarray(pos, np.float64).reshape(3)
    rays[:, 3:] = d
    state = np.zeros((1 + B, n), np.float64)
    if R == 0:
        state[1:] = (power * 1.0)[:, None]
        return rays, state
    table = np.asarray(gain, np.float64).reshape(6, R, R, B)
    F, iv, iu, p = lookup(d, np.eye(3) if frame is None else frame, R)
    if paths is not None:
        paths.update(p)
    state[1:] = (power[None, :] * table[F, iv, iu, :]).T
    return rays, state


# ---- the device cases (tests/test_gpu_source.py), shared with the CPU check that they are not vacuous (tests/test_source_api.py)
def rotation():
    """A proper rotation with no zero entry (about (1, 2, 3) by 0.7 rad)."""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * (K @ K)


FRAMES = {
    "identity": np.eye(3),
    "rotation": rotation(),
    "scaled_permutation": np.array([[0.0, 0.0, -2.5], [0.5, 0.0, 0.0], [0.0, 3.0, 0.0]]),
    "equal_rows": np.array([[0.3, -0.2, 0.9]] * 3),                                # a three-way tie for every ray
    "two_equal_rows": np.array([[1.0, 0, 0], [1.0, 0, 0], [0, 0, 1.0]]),             # a_0 = a_1 for every ray
    "rows_0_and_2_equal": np.array([[0, 1.0, 0], [1.0, 0, 0], [0, 1.0, 0]]),         # a_0 = a_2
    "rows_1_and_2_equal": np.array([[1.0, 0, 0], [0, 0, 1.0], [0, 0, 1.0]]),         # a_1 = a_2
    "zero": np.zeros((3, 3)),                                                      # 0 / 0: texel 0 of face 0
}
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097)
FIRST = (0, 2 ** 32 - 100, 2 ** 40)
BANDS = (1, 3, 8)
RES = (0, 1, 2, 16)
SEEDS = (0, -1, -2 ** 63)
POS = (1.25, -0.5, 3.0)


def table(R, B, seed=11):
    """A directivity table with every texel distinct, some zeros."""
    g = np.random.default_rng(seed).uniform(0.0, 2.0, (6, R, R, B))
    g.reshape(-1)[::7] = 0.0
    return g


def powers(B):
    return np.array([1.0, 0.5, 0.0, 3.0, 0.125, 1e-3, 7.0, 2.0])[:B].copy()


def reference(seed, first_ray, n, B, R, name, paths=None):
    """emit() of one device case: the source at POS with powers(B), table(R, B) read in FRAMES[name]."""
    return emit(seed, first_ray, n, POS, powers(B), FRAMES[name], R, table(R, B) if R else None, paths)
