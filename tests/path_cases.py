"""Inputs for the source paths' device tests (include/hare_hip.h, "Direct sound", "Image sources (first order)", "Image sources (second
order)"): case records built from numpy and the oracle alone, no GPU.  PathCase is the one record; reference(case) calls
tests.direct_ref.direct, tests.image_ref.image and tests.image2_ref.image2 as they are, for the orders the case runs.  The cases of those
three modules all stand in axis-aligned shoeboxes on dyadic coordinates, where the mirror's division, the float conversions of the FP32
pre-cull and most of the prune's arithmetic are exact; the cases here stand in OBLIQUE rooms: a base mesh (a tessellated shoebox, the box
of quadrilaterals, the baffle room, the partition room at 126 triangles), optionally a few polygons of tests.helpers.soup inside as
occluders, mapped by x -> A x + t with A = R diag(s), R a rotation from a unit quaternion and s per axis in [0.6, 1.7], the source and
the placed receivers mapped along.  Two sets.  edge_cases(): fixed and named, each with the class it is there for (`why`);
tests/test_path_cases.py asserts on the CPU that each holds it.  sweep_case(seed): one case drawn from a seed over the whole parameter
space (tools/fuzz_paths.py runs them by the thousand).  digest(result) is the SHA-256 that tests/golden/path_reference_digests.json pins
(tests/test_path_cases.py).  A directional case carries an ambisonic `order` (1, 2 or 3: 4, 9 or 16 channels); ambi_edge_cases() and
ambi_sweep_case(seed) at the end are the two sets again at orders 2 and 3 (tests/test_gpu_path_ambi.py), pinned in
tests/golden/path_ambi_reference_digests.json."""
import contextlib
import dataclasses
import functools
import hashlib
import json
import os

import numpy as np

import hare_amd.scenes as scenes
from oracle import pyoracle as po
from tests import ambi_ref
from tests import direct_ref as dr
from tests import image2_ref as i2
from tests import image_ref as ir
from tests.helpers import soup
from tests.scatter_ref import normals_of
from tests.source_ref import powers, table

ORDERS = ("direct", "image", "image2")
P_MAX = 300                              # polygons of a sweep case
KPP_MAX = 1_000_000                      # K x P x P where the second order runs: the reference's brute force and its per-path deposits stay about a second.
                                         # It cuts K to 11 at P = 300 and to 27 at P = 192: in the sweep the second order never meets K = 255 .. 257
                                         # (the first two orders do; the tile cases run the second order at P = 255 .. 513 with K = 4 and 8)
WORDS_MAX = 1 << 21                      # K x n_bins x B (x 4): 16 MiB of histogram per order
PARTITIONS = dr.PARTITIONS


@dataclasses.dataclass
class PathCase:
    name: str
    verts: np.ndarray                    # [P, 4, 3]
    nverts: np.ndarray                   # [P]
    partition: tuple                     # ("voxel", domain) | ("octree", depth, max_polys) | ("kdtree", depth, max_polys)
    pos: np.ndarray                      # the source: position [3]
    power: np.ndarray                    # [B]
    frame: np.ndarray                    # [3, 3] or None
    R: int                               # the gain table's resolution (0: none)
    gain: np.ndarray                     # [6, R, R, B] or None
    centers: np.ndarray                  # [K, 3]
    radii: np.ndarray                    # [K]
    map: bool                            # the receivers as a receiver map
    alpha: np.ndarray                    # [P, B] or None
    sigma: np.ndarray                    # [P, B] or None (only with alpha)
    frac_bits: int
    n_bins: int
    bin_len: float
    directional: bool
    n_weight: int
    orders: tuple                        # a non-empty subset of ORDERS
    image_cull: int = 1                  # scene option "image_cull"
    image2_prune: int = 1                # scene option "image2_prune"
    pair: tuple = ()                     # the options the edge test runs with 0 and with 1
    scene: str = ""                      # for describe() only
    why: str = ""                        # an edge case's class
    marks: dict = dataclasses.field(default_factory=dict)        # what the CPU test needs to find the class again (receiver and polygon numbers)
    order: int = 1                       # the ambisonic order of a directional case: 1, 2 or 3 (4, 9 or 16 channels)

    @property
    def K(self):
        return self.centers.shape[0]

    @property
    def P(self):
        return self.verts.shape[0]

    @property
    def B(self):
        return self.power.shape[0]

    @property
    def tables(self):
        return "none" if self.alpha is None else ("alpha" if self.sigma is None else "alpha+sigma")

    @property
    def shape(self):
        return (self.K, self.n_bins, self.B, ambi_ref.CHANNELS[self.order]) if self.directional else (self.K, self.n_bins, self.B)

    def describe(self):
        return (f"{self.name}: {self.scene} P={self.P} {' '.join(str(x) for x in self.partition)} K={self.K}{' map' if self.map else ''} B={self.B} "
                f"R={self.R} tables={self.tables} frac_bits={self.frac_bits} n_bins={self.n_bins} bin_len={self.bin_len!r}"
                f"{f' directional order={self.order}' if self.directional else ''} n_weight={self.n_weight} orders={'+'.join(self.orders)} "
                f"image_cull={self.image_cull} image2_prune={self.image2_prune} pos={self.pos.tolist()!r}")

    def without(self, **fields):
        return dataclasses.replace(self, **fields)


def oracle_of(case):
    """(oracle topology, oracle partition, normals [P, 3]) of a case."""
    To = po.Topology(case.verts, case.nverts)
    kind, *par = case.partition
    o = po.VoxelGrid([To], domain=par[0]) if kind == "voxel" else (po.Octree if kind == "octree" else po.KDTree)([To], *par)
    return To, o, normals_of(To)


_KEPT = {}


def reference(case, nthreads=16, keep=False):
    """What the library must return for the case, per order it runs: {"direct": dict(hist, det, seen, tallies), "image": the same and
    pairs, "image2": the same and cands, paths}, each onto zeros.  At order 2 or 3 each path order runs inside its own
    tests.ambi_ref.higher_order (an Extra collects every deposit made inside it) and the channels 4 .. C - 1 are joined behind the four.
    keep: kept under the case's name and served again (the fixed set, whose tests share it and leave it unchanged)."""
    if keep and case.name in _KEPT:
        return _KEPT[case.name]
    _, o, normals = oracle_of(case)
    src = (case.pos, case.power, case.frame, case.R, case.gain)
    tail = (case.centers, case.radii, case.n_weight, case.n_bins, case.bin_len, case.frac_bits)
    out = {}
    high = case.directional and case.order > 1
    for order in case.orders:
        hist, det, seen, tallies = np.zeros(case.shape[:3] + (4,) if high else case.shape, np.uint64), np.zeros((case.K, 2), np.uint64), {}, {}
        res = dict(hist=hist, det=det, seen=seen, tallies=tallies)
        with (ambi_ref.higher_order(case.order) if high else contextlib.nullcontext()) as extra:
            if order == "direct":
                dr.direct(o, *src, *tail, hist, det, seen, tallies, nthreads)
            elif order == "image":
                res["pairs"] = ir.image(o, case.verts, case.nverts, normals, *src, case.alpha, case.sigma, *tail, hist, det, seen, tallies, nthreads)
            else:
                res["cands"], res["paths"] = i2.image2(o, case.verts, case.nverts, normals, *src, case.alpha, case.sigma, *tail, hist, det, seen,
                                                       tallies, nthreads)
        if high:
            res["hist"] = ambi_ref.join(hist, extra)
        out[order] = res
    if keep:
        _KEPT[case.name] = out
    return out


def digest(out):
    """SHA-256 (hex) over a reference result: per order its name, hist, det and the counts."""
    h = hashlib.sha256()
    for order in ORDERS:
        if order not in out:
            continue
        res = out[order]
        h.update(f"{order} {res.get('pairs')} {res.get('cands')} {res.get('paths')}\n".encode())
        for name in ("hist", "det"):
            a = np.ascontiguousarray(res[name])
            h.update(f"{name} {a.dtype.str} {a.shape}\n".encode())
            h.update(a.tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def pinned_digests():
    """tests/golden/path_reference_digests.json: digest() of every edge case ("edge/" + name) and of the sweep's seeds ("sweep/" 0 .. 99)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_reference_digests.json")) as f:
        return json.load(f)


# ---- scenes
def room126():
    """The partition room of tests.receive_cases at 126 triangles: a 108-triangle shoebox with the wall at x = 5, y = 0 .. 4.2."""
    m = scenes.shoebox(nface=3)
    wall = scenes._patch([5.0, 0.0, 0.0], [0.0, 4.2, 0.0], [0.0, 0.0, 4.0], 3, 3)
    v = np.zeros((wall.shape[0], 4, 3))
    v[:, :3] = wall
    return np.concatenate([m.verts, v]), np.concatenate([m.nverts, np.full(wall.shape[0], 3, np.int32)]), m.size


DIRECT_PLACED = [((3.0, 2.0, 2.5), 0.25), ((3.125, 2.0, 1.5), 0.5), ((7.0, 2.0, 1.5), 0.3), ((0.5, 6.5, 3.5), 0.3), ((1.0, 6.0, 0.5), 0.0625)]


def base_scene(kind):
    """(verts, nverts, size, source position, placed receivers [(center, radius)]) of a base scene before the map: ("box", nface), "quads",
    "baffle" (tests.image_ref's, with tests.image2_ref's placed receivers) or "room" (tests.direct_ref's source and placed receivers)."""
    if kind == "room":
        v, nv, size = room126()
        return v, nv, size, np.array(dr.POS), DIRECT_PLACED
    if kind in ("quads", "baffle"):
        v, nv, size = ir.mesh_of(kind)
        return v, nv, size, np.array((2.0, 1.0, 1.0) if kind == "baffle" else ir.POS), [(c, r) for c, r, _ in i2.PLACED[kind]]
    m = scenes.shoebox(nface=kind[1])
    return m.verts, m.nverts, m.size, np.array(ir.POS), [(c, r) for c, r, _ in i2.PLACED["box12"]]


def occluders(n, seed, size, n_quad=None):
    """n polygons of tests.helpers.soup inside the box of `size` (every third a quadrilateral unless n_quad says otherwise), none of them
    the polygon that soup anchors at the origin."""
    if n <= 0:
        return np.zeros((0, 4, 3)), np.zeros(0, np.int32)
    nq = n // 3 if n_quad is None else n_quad
    v, nv, _ = soup(n_tri=n - nq + 1, n_quad=nq, seed=seed, size=size)
    keep = ~(v[:, 0] == 0.0).all(axis=1)
    v, nv = v[keep][:n], nv[keep][:n]
    assert v.shape[0] == n
    return v, nv


def quaternion_rotation(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def draw_map(rng, scale=1.0):
    """A = R diag(s) * scale: R from a drawn unit quaternion, s per axis from [0.6, 1.7]."""
    return (quaternion_rotation(rng.normal(size=4)) @ np.diag(rng.uniform(0.6, 1.7, 3))) * scale


class Mapped:
    """A mesh under x -> A x + t; t None: the mapped mesh's minimum corner goes to the origin (as tests.helpers.soup anchors
    it).  A quadrilateral's fourth corner is re-derived as v0 + (v2 - v1) behind the map, so that it stays planar to rounding."""

    def __init__(self, verts, nverts, A, t=None):
        self.A = np.asarray(A, np.float64)
        quad = nverts == 4
        v = verts @ self.A.T
        if t is None:
            t = -np.concatenate([v[:, :3].reshape(-1, 3), v[quad, 3]]).min(axis=0)
        self.t = np.asarray(t, np.float64)
        v = v + self.t
        v[quad, 3] = v[quad, 0] + (v[quad, 2] - v[quad, 1])
        v[~quad, 3] = 0.0
        self.verts, self.nverts = np.ascontiguousarray(v), np.ascontiguousarray(nverts, np.int32)

    def __call__(self, x):
        return np.asarray(x, np.float64) @ self.A.T + self.t

    @property
    def radius_scale(self):
        return float(abs(np.linalg.det(self.A)) ** (1.0 / 3.0))


def receivers_in(rng, m, size, K, placed):
    """K receivers: the placed ones mapped along (radii by the map's mean scale), the others drawn inside the mapped room."""
    c = m(rng.uniform(0.08, 0.92, (K, 3)) * np.asarray(size))
    r = rng.uniform(0.1, 0.3, K) * m.radius_scale
    for k, (ck, rk) in enumerate(placed[:K]):
        c[k], r[k] = m(ck), rk * m.radius_scale
    return np.ascontiguousarray(c), r


def tables_of(rng, kind, P, B):
    """(alpha, sigma) [P, B] or None, with some rows of 0 and of 1."""
    if kind == "none":
        return None, None
    alpha = rng.uniform(0.0, 0.7, (P, B))
    alpha[rng.random(P) < 0.1] = 0.0
    alpha[rng.random(P) < 0.05] = 1.0
    if kind == "alpha":
        return alpha, None
    sigma = rng.uniform(0.0, 0.8, (P, B))
    sigma[rng.random(P) < 0.1] = 0.0
    sigma[rng.random(P) < 0.05] = 1.0
    return alpha, sigma


def make(name, m, partition, pos, centers, radii, *, as_map=None, B=3, R=0, frame=None, tables="alpha", frac_bits=40, n_bins=64, bin_len=0.5,
         directional=False, n_weight=4097, orders=ORDERS, seed=0, **more):
    rng = np.random.default_rng(1000 + seed)
    P = m.verts.shape[0]
    centers, radii = np.ascontiguousarray(np.asarray(centers, np.float64).reshape(-1, 3)), np.asarray(radii, np.float64).reshape(-1)
    alpha, sigma = tables_of(rng, tables, P, B)
    if R and frame is None:
        frame = quaternion_rotation(rng.normal(size=4))
    return PathCase(name, m.verts, m.nverts, partition, np.asarray(pos, np.float64), powers(B), frame if R else None, R, table(R, B) if R else None,
                    centers, radii, centers.shape[0] > 256 if as_map is None else as_map, alpha, sigma, frac_bits, n_bins, bin_len, directional,
                    n_weight, tuple(orders), **more)


# ---- edge cases
V8, O48, T86 = PARTITIONS


def _box(nface, seed, extra=0, partition=V8, t=None, scale=1.0, n_quad=None, size=(10.0, 7.0, 4.0), walls_last=False):
    """An oblique shoebox of 12 nface^2 triangles and `extra` occluders: (Mapped, size, mapped source, base placed receivers, rng)."""
    rng = np.random.default_rng(7000 + seed)
    v, nv, size, pos, placed = base_scene(("box", nface))
    ov, onv = occluders(extra, seed, size, n_quad)
    parts = ((ov, v), (onv, nv)) if walls_last else ((v, ov), (nv, onv))
    m = Mapped(np.concatenate(parts[0]), np.concatenate(parts[1]), draw_map(rng, scale), t)
    return m, size, m(pos), placed, rng


def tile_cases():
    """P exactly 255, 256, 257 and 513 in an oblique room: the pair search's blocks of 256 polygons and the candidate stage's tiles of 256
    second polygons, full, one short, one over and two and a bit; K = 255 and 256 linear and 257 as a map (the linear receivers end at
    256) with the first two orders, K = 8 with the second; receivers 3 .. 7 lie on paths off the last polygon (_via_last).  The occluders come first, so that the last polygons -- the one or
    two of a last partial block or tile -- are walls of the room, which paths do reflect off."""
    out = []
    for j, (P, nface, K) in enumerate(((255, 4, 255), (256, 4, 256), (257, 4, 257), (513, 6, 257))):
        m, size, pos, placed, rng = _box(nface, (10, 31, 12, 13)[j], P - 12 * nface * nface, partition=PARTITIONS[j % 3], walls_last=True)
        c, r = receivers_in(rng, m, size, K, placed)
        c[3:8], r[3:8] = _via_last(m, pos), 0.1
        out.append(make(f"P{P}-K{K}", m, PARTITIONS[j % 3], pos, c, r, B=(1, 3, 8, 3)[j], R=(0, 4, 0, 1)[j], tables=("alpha", "alpha+sigma", "none", "alpha")[j],
                        n_bins=32, bin_len=1.0, directional=j % 2 == 1, orders=("direct", "image"), seed=j, scene=f"box{nface}+soup",
                        why="P and K about a block of 256"))
        K2 = 8
        out.append(make(f"P{P}-K{K2}-second", m, PARTITIONS[j % 3], pos, c[:K2], r[:K2], B=(3, 1, 3, 1)[j], tables="alpha", n_bins=64, bin_len=1.0,
                        directional=j % 2 == 0, orders=("image2",), pair=("image2_prune",), seed=j, scene=f"box{nface}+soup",
                        why="P about a tile of 256 second polygons"))
    return out


def _mirror_dir(d, n):
    return d - n * (2.0 * np.dot(d, n) / np.dot(n, n))


def _via_last(m, S):
    """Five centers on paths off the centroid of the mesh's LAST polygon: one reflected there (first order), one whose first reflection
    is there (second order, as p), three whose second reflection is there behind a first one in some other polygon (as q)."""
    To = po.Topology(m.verts, m.nverts)
    n = normals_of(To)
    last = m.verts.shape[0] - 1
    x = m.verts[last, :3].mean(axis=0)
    u = _mirror_dir(x - S, n[last])
    unit = lambda a: a / np.linalg.norm(a)
    out = [x + unit(u) * 0.5]
    _, x2, u2 = _first_hit(To, n, x + u * 1e-9, u)
    _, x3, _ = _first_hit(To, n, x2 + u2 * 1e-9, u2)
    out.append(x2 + (x3 - x2) * 0.5)
    S1, mirrored, _ = ir.mirror(S, m.verts, n)
    w = x[None] - S1
    hit, t = i2.poly_fast_rows(S1, w, m.verts, m.nverts, n)
    ps = np.nonzero(hit & (t > 0.0) & (t < 1.0) & mirrored & (np.arange(last + 1) != last))[0]
    ps = ps[np.linspace(0, ps.size - 1, 3).astype(int)]
    return np.array(out + [x + unit(_mirror_dir(w[p], n[last])) * 0.5 for p in ps])


def d2_of(c, s):
    v = np.asarray(c, np.float64) - np.asarray(s, np.float64)
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def radius_at(c0, s, rel):
    """(center, radius) next to c0 with d2 = |center - s|^2, as the definition rounds it, and rr = radius * radius in the relation `rel`:
    ">" d2 == nextafter(rr, +inf), "=" d2 == rr, "<" d2 == nextafter(rr, -inf).  Not every double is a square, so the center moves by
    a few units in the last place until one fits."""
    c0 = np.asarray(c0, np.float64)
    for i in range(600):
        c = c0.copy()
        for _ in range(i // 3):
            c[i % 3] = np.nextafter(c[i % 3], np.inf)
        d2 = d2_of(c, s)
        rr = {">": np.nextafter(d2, -np.inf), "=": d2, "<": np.nextafter(d2, np.inf)}[rel]
        r = np.sqrt(rr)
        for _ in range(3):
            r = np.nextafter(r, -np.inf)
        for _ in range(7):
            if r * r == rr:
                return c, float(r)
            r = np.nextafter(r, np.inf)
    raise AssertionError("no radius found")


def rr_case():
    """For each order a receiver whose d2 towards S, an S' and an S'' is nextafter(rr, +inf), exactly rr and nextafter(rr, -inf): the
    eligibility comparison d2 > rr, and the share at x = rr / d2 next to 1, where sqrt(1 - x) is tiny or 0."""
    m, size, pos, placed, rng = _box(1, 20)
    case0 = make("probe", m, V8, pos, m(rng.uniform(0.2, 0.8, (9, 3)) * np.asarray(size)), np.full(9, 1e-3), tables="none", orders=("image", "image2"))
    ref = reference(case0)
    s1, s2 = ref["image"]["seen"], ref["image2"]["seen"]
    c, r, marks = case0.centers.copy(), np.zeros(9), {}
    for j, rel in enumerate((">", "=", "<")):
        c[j], r[j] = radius_at(c[j], pos, rel)
        k = 3 + j
        i = np.nonzero((s1["k"] == k) & ~s1["occ_rcv"] & ~s1["occ_src"])[0][0]
        c[k], r[k] = radius_at(c[k], s1["S"][s1["p"][i]], rel)
        marks[k] = (int(s1["p"][i]),)
        k = 6 + j
        i = np.nonzero((s2["k"] == k) & ~s2["occ"].any(axis=1))[0][0]
        p, q = int(s2["p"][i]), int(s2["q"][i])
        cd = s2["cands"]
        c[k], r[k] = radius_at(c[k], cd["S2"][np.nonzero((cd["p"] == p) & (cd["q"] == q))[0][0]], rel)
        marks[k] = (p, q)
    return make("rr-edges", m, V8, pos, c, r, B=3, R=4, tables="alpha+sigma", n_bins=64, bin_len=1.0, directional=True, scene="box1",
                why="d2 one ulp either side of rr and on it, per order", marks=marks)


def plane_cases():
    """The source in an oblique polygon's plane as far as FP64 allows -- at that polygon's v0, where h == 0 exactly, while the coplanar
    neighbours, whose h goes through their own v0, get an h of rounding's size or 0 -- and one ulp off it (h tiny and nonzero: mirrored,
    S' ~ S)."""
    rng = np.random.default_rng(7030)
    v, nv, size, _, placed = base_scene("baffle")
    m = Mapped(v, nv, draw_map(rng))
    p = next(i for i in range(48, 56) if np.allclose(v[i, 0], (5.0, 1.25, 2.0)))      # a baffle triangle whose v0 is the baffle's middle vertex
    c, r = receivers_in(rng, m, size, 12, placed)
    at = m.verts[p, 0].copy()
    out = [make("source-in-plane", m, T86, at, c, r, B=3, tables="alpha", bin_len=0.5, scene="baffle", pair=("image_cull", "image2_prune"),
                why="h == 0 at one polygon, rounding's size at its coplanar neighbours", marks=dict(p=p))]
    n = normals_of(po.Topology(m.verts, m.nverts))[p]
    a = int(np.argmax(np.abs(n)))
    off = at.copy()
    off[a] = np.nextafter(off[a], np.inf)
    out.append(make("source-ulp-off-plane", m, O48, off, c, r, B=1, R=4, tables="alpha+sigma", bin_len=0.5, directional=True, scene="baffle",
                    pair=("image_cull", "image2_prune"), why="h tiny and nonzero: S' ~ S", marks=dict(p=p)))
    return out


def coplanar_case():
    """Coplanar neighbours p, q in an oblique plane: h2 is -h up to the rounding through q's own v0; whether S'' exists, and where, is a
    matter of bits."""
    m, size, pos, placed, rng = _box(3, 40, partition=O48)
    c, r = receivers_in(rng, m, size, 8, placed)
    return make("coplanar-neighbours", m, O48, pos, c, r, B=3, tables="alpha", bin_len=0.5, scene="box3", pair=("image2_prune",),
                why="h2 == -h up to rounding among a wall's triangles")


def with_polys(m0_verts, m0_nverts, extra):
    v = np.zeros((len(extra), 4, 3))
    for i, tri in enumerate(extra):
        v[i, :3] = tri
    return np.concatenate([m0_verts, v]), np.concatenate([m0_nverts, np.full(len(extra), 3, np.int32)])


def prune_cases():
    """The prune's limits, each with the prune 0 and 1: the source within 1e-7 of a large polygon's interior (cosm <= 1e-6: no prune for
    that p); the source far from a small polygon (a narrow cone) and a sliver of aspect 1000 : 1 as p and as q; a polygon with a NaN-free
    but huge bounding sphere."""
    out = []
    rng = np.random.default_rng(7050)
    v, nv, size, pos, placed = base_scene(("box", 1))
    m = Mapped(v, nv, draw_map(rng))
    n = normals_of(po.Topology(m.verts, m.nverts))
    g = m.verts[0, :3].mean(axis=0)
    inward = np.sign(np.dot(m(np.asarray(size) / 2) - g, n[0]))
    c, r = receivers_in(rng, m, size, 8, placed)
    out.append(make("prune-source-on-wall", m, V8, g + n[0] * (inward * 1e-7), c, r, B=3, tables="alpha", scene="box1", pair=("image2_prune", "image_cull"),
                    why="cosm <= 1e-6 for the polygon under the source", marks=dict(p=0)))
    small = [(8.0, 5.0, 2.0), (8.01, 5.0, 2.0), (8.0, 5.01, 2.0)]
    sliver = [(4.0, 4.0, 1.5), (6.0, 4.0, 1.5), (5.0, 4.0005, 1.5)]
    v2, nv2 = with_polys(*base_scene(("box", 2))[:2], [small, sliver])
    m = Mapped(v2, nv2, draw_map(rng))
    c, r = receivers_in(rng, m, size, 8, placed)
    n = normals_of(po.Topology(m.verts, m.nverts))
    S = m((1.0, 1.0, 1.0))
    for k, p in enumerate((48, 49)):                                    # receivers 0 and 1 on the paths reflected in the two polygons' centroids
        x = m.verts[p, :3].mean(axis=0)
        d = x - S
        c[k], r[k] = x + (d - n[p] * (2.0 * np.dot(d, n[p]) / np.dot(n[p], n[p]))) * 0.2, 0.05
    out.append(make("prune-small-and-sliver", m, T86, S, c, r, B=3, R=1, tables="alpha+sigma", scene="box2+2", pair=("image2_prune",),
                    why="a narrow cone; a sliver 1000 : 1 as p and as q", marks=dict(small=48, sliver=49)))
    huge = [(-4000.0, -4000.0, -2.0), (9000.0, -3000.0, -2.0), (1000.0, 9000.0, -2.0)]
    v3, nv3 = with_polys(*base_scene(("box", 2))[:2], [huge])
    m = Mapped(v3, nv3, draw_map(rng), t=np.zeros(3))
    c, r = receivers_in(rng, m, size, 8, placed)
    out.append(make("prune-huge-sphere", m, T86, m(pos), c, r, B=1, tables="alpha", scene="box2+huge", pair=("image2_prune", "image_cull"),
                    why="a bounding sphere a thousand rooms wide", marks=dict(huge=48)))
    return out


def prune_margin_case():
    """The prune's plane test with nothing to spare: a long triangle q that stands on the baffle's plane like a nail, its tip -- the corner
    farthest from its centroid -- 1 cm on the source's side, the rest 3 m behind the plane.  q's bounding sphere reaches through p's
    plane by 0.5 % of its radius, and the only second reflection points of (p, q) lie in that tip.  Receiver 0 is on such a path.  A prune
    whose sphere is 1 % small drops the candidate; the margin of the real one (1e-9, relative) must not."""
    rng = np.random.default_rng(7057)
    v, nv, size, pos, placed = base_scene("baffle")
    m = m0 = Mapped(v, nv, draw_map(rng))
    S = m(pos)
    n = normals_of(po.Topology(m.verts, m.nverts))
    p = 50
    x0 = m.verts[p, :3].mean(axis=0)
    unit = lambda a: a / np.linalg.norm(a)
    ns = unit(n[p]) * np.sign(np.dot(S - x0, n[p]))                     # p's unit normal towards the source
    t = unit(m.verts[p, 1] - m.verts[p, 0])
    A, B, C = x0 + ns * 0.01, x0 - ns * 3.0 + t * 0.1, x0 - ns * 3.0 - t * 0.1
    m = Mapped(*with_polys(m.verts, m.nverts, [(A, B, C)]), np.eye(3), np.zeros(3))
    q = m.verts.shape[0] - 1
    n = normals_of(po.Topology(m.verts, m.nverts))
    x2 = A + ((A + B + C) / 3.0 - A) * 0.002
    S1 = ir.mirror(S, m.verts, n)[0][p]
    c, r = receivers_in(rng, m0, size, 8, placed)
    c[0], r[0] = x2 + unit(_mirror_dir(x2 - S1, n[q])) * 0.5, 0.05
    return make("prune-plane-margin", m, V8, S, c, r, B=3, tables="alpha", bin_len=0.5, scene="baffle+nail", pair=("image2_prune",),
                why="q's sphere reaches through p's plane by 0.5 % of its radius, and the path's x2 lies there", marks=dict(p=p, q=q))


def cull_cases():
    """The pre-cull's limits, each with image_cull 0 and 1: a room scaled by 1e-3 and by 1e3 (RayXtri's absolute |det| > 1e-6 rejects or
    accepts whole classes of polygons); a room whose minimum corner lies 1e4 m from the origin; receivers whose segment from S' and from
    S'' grazes a polygon's edge within 1e-9 of its length, one either side."""
    out = []
    for j, (tag, scale) in enumerate((("1e-3", 1e-3), ("1e3", 1e3))):
        m, size, pos, placed, rng = _box(2, 60, extra=6, scale=scale)
        c = m(np.random.default_rng(61).uniform(0.08, 0.92, (8, 3)) * np.asarray(size))
        out.append(make(f"cull-scale-{tag}", m, V8, pos, c, np.full(8, 0.2 * scale), B=3, tables="alpha", bin_len=0.5 * scale, scene="box2+soup",
                        pair=("image_cull", "image2_prune"), why=f"the room scaled by {tag}", marks=dict(scale=scale)))
    t = np.array([1.0e4, -1.0e4, 1.0e4])
    rng = np.random.default_rng(7062)
    v, nv, size, pos, placed = base_scene("quads")
    ov, onv = occluders(6, 62, size)
    m = Mapped(np.concatenate([v, ov]), np.concatenate([nv, onv]), draw_map(rng))
    m = Mapped(np.concatenate([v, ov]), np.concatenate([nv, onv]), m.A, m.t + t)
    c, r = receivers_in(rng, m, size, 8, placed)
    out.append(make("cull-far-from-origin", m, V8, m(pos), c, r, B=3, R=4, tables="alpha+sigma", directional=True, scene="quads+soup",
                    pair=("image_cull", "image2_prune"), why="the minimum corner 1e4 m from the origin"))
    # grazing: the baffle's free edge at y = 2.5 (its polygons 48 .. 55), from S' of a baffle polygon and from S'' of (p, that polygon)
    rng = np.random.default_rng(7063)
    v, nv, size, pos, placed = base_scene("baffle")
    m = Mapped(v, nv, draw_map(rng))
    S = m(pos)
    probe = make("probe", m, V8, S, m(((6.0, 1.0, 1.0),)), (0.1,), tables="none", orders=("image2",))
    normals = oracle_of(probe)[2]
    q = next(i for i in range(48, 56) if (np.isclose(v[i, :3, 1], 2.5).sum() == 2))
    a, b = (m.verts[q, i] for i in range(3) if np.isclose(v[q, i, 1], 2.5))
    e = a + (b - a) * 0.37
    inw = m.verts[q, :3].mean(axis=0) - e                               # from the edge into the polygon
    S1 = ir.mirror(S, m.verts, normals)[0]
    cd = i2.candidates(S, m.verts, normals)
    def graze(origin):                                                  # two centers behind the edge: the segment from `origin` passes 1e-9 of its length inside q, and outside
        L = np.linalg.norm(e - origin)
        return [origin + ((e + inw * (sgn * 1e-9 * L / np.linalg.norm(inw))) - origin) * 1.6 for sgn in (1.0, -1.0)]

    def whole_path(i):                                                  # candidate i's path reaches the inside center with every leg free, and not the outside one
        s = reference(make("probe", m, V8, S, graze(cd["S2"][i]), (0.05, 0.05), tables="none", orders=("image2",)))["image2"]["seen"]
        at = (s["p"] == cd["p"][i]) & (s["q"] == q)
        return ((s["k"] == 0) & at & ~s["occ"].any(axis=1)).any() and not ((s["k"] == 1) & at).any()

    i2nd = next(i for i in np.nonzero(cd["q"] == q)[0] if whole_path(i))
    centers = graze(S1[q]) + graze(cd["S2"][i2nd])
    marks = {0: ("first", True), 1: ("first", False), 2: ("second", True), 3: ("second", False), "q": q, "p2": int(cd["p"][i2nd])}
    rest, rr = receivers_in(rng, m, size, 4, [])
    out.append(make("cull-grazing-edge", m, V8, S, np.concatenate([np.array(centers), rest]), np.concatenate([np.full(len(centers), 0.05), rr]), B=1,
                    tables="alpha", bin_len=0.5, scene="baffle", pair=("image_cull",), why="segments from S' and S'' within 1e-9 of an edge", marks=marks))
    return out


def _first_hit(To, normals, o, d):
    ev = po.brute(To, np.concatenate([o, d])[None])
    ev = ev[0] if isinstance(ev, tuple) else ev
    assert int(ev["hit"][0]) == 1
    p = int(ev["poly_id"][0])
    x = o + d * float(ev["t"][0])
    n = normals[p]
    return p, x, d - n * (2.0 * np.dot(d, n) / np.dot(n, n))


def table_cases():
    """A source table with R = 1 and R = 4 in a rotated frame, with leave directions on a cube-face edge and on a cube corner of the
    source's frame: towards a receiver (direct), towards the reflection point of a first-order path and towards the first reflection point
    of a second-order one -- the direction is constructed, then followed off the walls to where the receiver goes."""
    out = []
    for j, R in enumerate((1, 4)):
        m, size, pos, placed, rng = _box(2, 80 + j)
        frame = quaternion_rotation(rng.normal(size=4))
        To = po.Topology(m.verts, m.nverts)
        normals = normals_of(To)
        centers, marks = [], {}
        for tag, local in (("edge", (1.0, 1.0, 0.25)), ("corner", (1.0, -1.0, 1.0)), ("edge", (-1.0, 0.5, -1.0)), ("corner", (-1.0, -1.0, -1.0))):
            d = frame.T @ np.asarray(local)                             # l = frame d gives `local` back, to rounding
            d = d / np.linalg.norm(d)
            for order in ORDERS:
                o, u = pos, d
                for _ in range(ORDERS.index(order)):
                    _, o, u = _first_hit(To, normals, o, u)
                    o = o + u * 1e-9
                p, x, _ = _first_hit(To, normals, o, u)
                marks[len(centers)] = (order, tag)
                centers.append(o + (x - o) * 0.5 if order != "direct" else pos + d * (np.linalg.norm(x - pos) * 0.5))
        K = len(centers)
        out.append(make(f"table-R{R}-edges", m, PARTITIONS[j], pos, np.array(centers), np.full(K, 0.2), B=3, R=R, frame=frame, tables="alpha",
                        bin_len=0.5, directional=j == 1, scene="box2", why="leave directions on the cube map's edges and corners", marks=marks))
    return out


@functools.lru_cache(maxsize=None)
def edge_cases():
    out = tile_cases() + [rr_case()] + plane_cases() + [coplanar_case()] + prune_cases() + [prune_margin_case()] + cull_cases() + table_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def variants(case):
    """The case with every combination of the options its `pair` names at 0 and 1 (the case alone without a pair)."""
    out = [case]
    for opt in case.pair:
        out = [c.without(**{opt: v}) for c in out for v in (0, 1)]
    return out


# ---- sweep cases
def sweep_case(seed):
    """One case from the seed.  Nothing is redrawn: every draw is accepted as it comes; K and n_bins are cut to the caps."""
    rng = np.random.default_rng(0x9A7B0000 + int(seed))
    which = int(rng.integers(0, 7))
    kind = (("box", 1), ("box", 2), ("box", 3), ("box", 4), "quads", "baffle", "room")[which]
    v, nv, size, pos, placed = base_scene(kind)
    n_occ = int(rng.integers(0, 9)) if rng.random() < 0.6 else 0
    ov, onv = occluders(n_occ, int(rng.integers(0, 1000)), size)
    verts, nverts = np.concatenate([v, ov]), np.concatenate([nv, onv])
    part = ("voxel", "octree", "kdtree")[int(rng.integers(0, 3))]
    if part == "voxel":
        partition = ("voxel", int(rng.choice([1, 2, 5, 8, 13])))
    elif part == "octree":
        partition = ("octree", int(rng.integers(0, 3)), int(rng.integers(1, 40)))
    else:
        partition = ("kdtree", int(rng.integers(0, 11)), int(rng.integers(1, 40)))
    A = draw_map(rng)
    t = rng.uniform(-1000.0, 1000.0, 3)
    m = Mapped(verts, nverts, A, None if part == "octree" or rng.random() < 0.3 else t)
    P = m.verts.shape[0]
    assert P <= P_MAX
    orders = tuple(o for o in ORDERS if rng.random() < 0.6) or ORDERS
    r = rng.random()
    K = 1 if r < 0.15 else 8 if r < 0.35 else int(rng.integers(255, 258)) if r < 0.55 else int(rng.integers(1, 301))
    if "image2" in orders:
        K = max(1, min(K, KPP_MAX // (P * P)))
    B = int(rng.integers(1, 9))
    R = int(rng.choice([0, 1, 4]))
    directional = bool(rng.integers(0, 2))
    n_bins = int(np.exp(rng.uniform(0.0, np.log(2001.0))))
    n_bins = max(1, min(n_bins, WORDS_MAX // (K * B * (4 if directional else 1))))
    bin_len = float(np.exp(rng.uniform(np.log(1e-3), np.log(10.0))))
    if rng.random() < 0.5:                                              # half of the histograms reach across the room twice
        bin_len = max(bin_len, 40.0 / n_bins)
    c, rad = receivers_in(rng, m, size, K, placed if rng.random() < 0.7 else [])
    src = m(pos) if rng.random() < 0.5 else m(rng.uniform(0.1, 0.9, 3) * np.asarray(size))
    return make(f"sweep-{seed}", m, partition, src, c, rad, as_map=K > 256 or bool(rng.random() < 0.2), B=B, R=R,
                tables=("none", "alpha", "alpha+sigma")[int(rng.integers(0, 3))], frac_bits=int(rng.integers(0, 63)), n_bins=n_bins, bin_len=bin_len,
                directional=directional, n_weight=(1, 4097, 2 ** 40)[int(rng.integers(0, 3))], orders=orders, seed=int(seed),
                image_cull=int(rng.integers(0, 2)), image2_prune=int(rng.integers(0, 2)), scene=f"{kind}+{n_occ}")


# ---- the higher orders: nine and sixteen channels (tests/test_gpu_path_ambi.py)
@functools.lru_cache(maxsize=None)
def pinned_ambi_digests():
    """tests/golden/path_ambi_reference_digests.json: digest() of every ambi edge case ("edge/" + name) and, for the ambi sweep's seeds
    ("sweep/" 0 .. N - 1), dict(digest, higher: whether channels 4 .. C - 1 hold a non-zero word in some order)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_ambi_reference_digests.json")) as f:
        return json.load(f)


def higher_nonzero(out):
    return bool(any(res["hist"][..., 4:].any() for res in out.values()))


AXIS_SIZE = (10.0, 7.0, 4.0)


def axis_box(name, order, *, frac_bits=40, power=None, why=""):
    """The 12-triangle shoebox UNMAPPED (A the identity, every coordinate dyadic), the source at (3, 2, 1), and receivers of radius 1/8 on
    the lattice of whole metres inside: the vectors from S, from the six S' and from the S'' to them have whole components, among them
    (a, 0, 0), (a, a, 0) and (a, a, a) in every sign and axis -- arrivals along the axes, the face diagonals and the space diagonals, their
    components 0, +-1, +-sqrt(1/2) and +-sqrt(1/3) as the division by dist leaves them -- and whole layers of receivers at the height of
    the source and of its images behind the walls, where az == 0 and so Y6 == -0.5 exactly.  Receiver 0 is (5, 4, 1): its direct path
    arrives along (-1, -1, 0) / sqrt(2)."""
    v, nv, size, pos, _ = base_scene(("box", 1))
    m = Mapped(v, nv, np.eye(3), np.zeros(3))
    c = [(5.0, 4.0, 1.0)] + [(x, y, z) for x in (1.0, 3.0, 5.0, 7.0) for y in (1.0, 2.0, 4.0, 6.0) for z in (1.0, 2.0, 3.0) if (x, y, z) not in ((5.0, 4.0, 1.0), (3.0, 2.0, 1.0))]
    case = make(name, m, V8, pos, np.array(c), np.full(len(c), 0.125), B=3, tables="none", frac_bits=frac_bits, n_bins=64, bin_len=0.5, directional=True,
                scene="box1 unmapped", why=why, order=order)
    return case if power is None else case.without(power=np.asarray(power, np.float64))


def tie_powers(frac_bits, targets=(1.0, 3.0, 5.0)):
    """power [3] with m_b = (power_b * fw) * 2^frac_bits EXACTLY 1, 3 and 5 on the direct path of axis_box's receiver 0 (no table, no
    reflectance: the deposit's products with 1.0 are exact): the quotient, moved by units in the last place until the product is the
    target.  m_b * Y6 is then -0.5, -1.5 and -2.5, ties of the rint, and rint(m_b) 1, 3 and 5."""
    case = axis_box("probe", 3)
    fw = dr.share(case.radii[0] * case.radii[0], d2_of(case.centers[0], case.pos)) * np.float64(case.n_weight)
    out = []
    for t in targets:
        p = np.float64(t) / (fw * np.float64(2.0 ** frac_bits))
        for _ in range(64):
            got = (p * fw) * np.float64(2.0 ** frac_bits)
            if got == t:
                break
            p = np.nextafter(p, np.inf if got < t else -np.inf)
        assert (p * fw) * np.float64(2.0 ** frac_bits) == t, (t, p)
        out.append(p)
    return np.array(out)


def drum_room(n_side=64, radius=4.0, height=3.0):
    """A prism over a regular n_side-gon: n_side wall quadrilaterals, each in a plane of its own, a floor and a ceiling of n_side triangles
    each about the axis.  From a source and receivers near the axis every wall reflects a first-order path and every (wall, floor),
    (floor, wall), (wall, ceiling), (ceiling, wall) pair a second-order one -- the 6 planes of a shoebox give 6 and about 30, however
    finely they are tessellated."""
    a = 2.0 * np.pi * np.arange(n_side + 1) / n_side
    ring = np.stack([radius + radius * np.cos(a), radius + radius * np.sin(a)], axis=1)
    v, nv = np.zeros((3 * n_side, 4, 3)), np.full(3 * n_side, 3, np.int32)
    for i in range(n_side):
        (x0, y0), (x1, y1) = ring[i], ring[i + 1]
        v[i] = [(x0, y0, 0.0), (x1, y1, 0.0), (x1, y1, height), (x0, y0, height)]
        v[n_side + i, :3] = [(radius, radius, 0.0), (x0, y0, 0.0), (x1, y1, 0.0)]
        v[2 * n_side + i, :3] = [(radius, radius, height), (x0, y0, height), (x1, y1, height)]
    nv[:n_side] = 4
    return v, nv, (2.0 * radius, 2.0 * radius, height)


def one_word_case():
    """Every path of a receiver into ONE bin (n_bins = 1, bin_len 1000): each of its B x 16 words is the wrapped sum of one atomic per
    path -- more than 50 first-order and 200 second-order paths per receiver in the drum room, rotated by a drawn quaternion and scaled
    by 1.3 on every axis (a map that keeps angles, so that the walls go on reflecting towards the axis)."""
    rng = np.random.default_rng(7090)
    v, nv, size = drum_room()
    m = Mapped(v, nv, quaternion_rotation(rng.normal(size=4)) * 1.3)
    mid = np.asarray(size) / 2
    c = m(mid + np.array([(0.15, 0.05, 0.1), (-0.1, 0.125, -0.2), (0.05, -0.15, 0.25), (-0.125, -0.1, -0.05)]))
    return make("one-word-o3", m, V8, m(mid + np.array((0.075, -0.05, 0.15))), c, np.full(4, 0.1 * m.radius_scale), B=3, tables="alpha", frac_bits=40,
                n_bins=1, bin_len=1000.0, directional=True, scene="drum64", why="many paths of a receiver in one word", order=3)


def wide_cases():
    """B = 8 at order 3, 128 words per deposit: K = 255 and 256 linear and 257 as a map with the first two orders; K = 8 with the second
    order at P = 256."""
    out = []
    for j, K in enumerate((255, 256, 257)):
        m, size, pos, placed, rng = _box(2, 90 + j, extra=6, partition=PARTITIONS[j])
        c, r = receivers_in(rng, m, size, K, placed)
        out.append(make(f"wide-K{K}-o3", m, PARTITIONS[j], pos, c, r, B=8, R=(0, 4, 1)[j], tables=("alpha", "alpha+sigma", "none")[j], n_bins=32, bin_len=1.0,
                        directional=True, orders=("direct", "image"), seed=j, scene="box2+soup", why="128 words per deposit, K about a block of 256", order=3))
    m, size, pos, placed, rng = _box(4, 31, 256 - 192, partition=O48, walls_last=True)
    c, r = receivers_in(rng, m, size, 8, placed)
    out.append(make("wide-P256-K8-second-o3", m, O48, pos, c, r, B=8, tables="alpha", n_bins=64, bin_len=1.0, directional=True, orders=("image2",),
                    pair=("image2_prune",), scene="box4+soup", why="128 words per deposit, P a tile of 256 second polygons", order=3))
    return out


def partition_cases3():
    out = []
    for j, part in enumerate(PARTITIONS):
        m, size, pos, placed, rng = _box(2, 95 + j, extra=8, partition=part)
        c, r = receivers_in(rng, m, size, 8, placed)
        out.append(make(f"{part[0]}-o3", m, part, pos, c, r, B=3, R=(4, 0, 1)[j], tables="alpha+sigma", bin_len=0.5, directional=True, seed=j,
                        scene="box2+soup", why=f"order 3 under the {part[0]} partition, with occluders", order=3))
    return out


@functools.lru_cache(maxsize=None)
def ambi_edge_cases():
    """The fixed cases of the nine- and sixteen-channel forms: every directional case of edge_cases() again at order 2 and 3 (name +
    "-o2" / "-o3"; the option pairs run through variants() as before); arrivals along the axes and diagonals (axis_box); ties of the
    signed words and the clamp; the widest word block; many paths in one word; every partition."""
    out = [c.without(name=f"{c.name}-o{o}", order=o, marks=dict(c.marks, base=c.name)) for c in edge_cases() if c.directional for o in (2, 3)]
    for o in (2, 3):
        out.append(axis_box(f"arrivals-o{o}", o, why="arrivals along the axes, the face diagonals and the space diagonals; az == 0"))
        for fb in (0, 1):
            out.append(axis_box(f"ties-f{fb}-o{o}", o, frac_bits=fb, power=tie_powers(fb), why="m = 1, 3, 5 with Y6 == -0.5: the signed words' ties"))
        out.append(axis_box(f"clamp-f62-o{o}", o, frac_bits=62, power=np.full(3, 2.0 ** 20), why="m == 2^63: every signed channel at the +-2^62 clamp"))
    out += wide_cases() + [one_word_case()] + partition_cases3()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


AMBI_KBC_MAX = 8192                      # K x B x C of an ambi sweep case: the reference makes B x (C - 1) numpy adds per path and a receiver has some
                                         # six first-order paths, so the slowest seeds stay at a few seconds (K = 64 at B = 8, C = 16; the wide
                                         # cases of ambi_edge_cases() run K = 255 .. 257 there)


def ambi_sweep_case(seed):
    """sweep_case(seed), directional, at an order drawn from a generator of its own (the base draw is untouched): 2 or 3.  Three rules,
    each a function of the base case alone; no seed is skipped or redrawn.
    K is cut to AMBI_KBC_MAX / (B C) receivers (the first ones: the placed receivers stay).
    To stay within WORDS_MAX words per order at 9 or 16 channels n_bins is halved (rounded up) and bin_len doubled until
    K x n_bins x B x C fits: the histogram covers the base seed's time span (one bin more where n_bins was odd), so every path the base
    seed bins is binned here.
    A quarter of the base seeds draw a histogram that ends before the NEAREST receiver's direct distance |c - S|, which no path of any
    order undercuts: every arrival is counted as unbinned and the histogram stays zero on all channels, whatever frac_bits is.  Those
    seeds alone get bin_len doubled until the histogram reaches past the FARTHEST receiver's direct distance; a histogram that bins
    anything keeps its span, short ones with unbinned arrivals included.  frac_bits stays the base seed's: with that rule
    tests/test_path_cases.py finds the channels 4 .. C - 1 all zero in fewer than 10 of 100 seeds (low frac_bits rounding every m * Y
    to 0), so the draw needed no change."""
    base = sweep_case(seed)
    order = int(np.random.default_rng(0xA3B20000 + int(seed)).integers(2, 4))
    C = ambi_ref.CHANNELS[order]
    K = max(1, min(base.K, AMBI_KBC_MAX // (base.B * C)))
    centers, radii = np.ascontiguousarray(base.centers[:K]), base.radii[:K]
    n_bins, bin_len = base.n_bins, base.bin_len
    while K * n_bins * base.B * C > WORDS_MAX:
        n_bins, bin_len = (n_bins + 1) // 2, bin_len * 2.0
    d = np.sqrt(((centers - base.pos[None]) ** 2).sum(axis=1))
    if n_bins * bin_len < d.min():
        while n_bins * bin_len <= d.max():
            bin_len *= 2.0
    return base.without(name=f"ambi-sweep-{seed}", directional=True, order=order, centers=centers, radii=radii, n_bins=n_bins, bin_len=bin_len)
