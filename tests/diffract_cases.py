"""The device cases of first-order edge diffraction (tests/test_gpu_diffract.py) and their reference (tests/diffract_ref.py), shared with
the CPU checks that each case holds the class it names (tests/test_diffract_cases.py) and that the reference stays what it is
(tests/test_diffract_reference_pinned.py).  Two scenes in the 10 x 7 x 4 shoebox of 12 triangles: "screen", one quadrilateral standing on
the floor at x = 5 (polygon 12) with its three free edges, faces (12, -1); "wedge", a box obstacle of six quadrilaterals (polygons 12 ..
17) with its twelve edges, two faces each.  sweep_case(seed) draws screens, an obstacle, source, receivers, bands, order and partition."""
import dataclasses
import hashlib

import numpy as np

from hare_amd import scenes
from oracle import pyoracle as po
from tests import ambi_ref
from tests import diffract_ref as dr
from tests.source_ref import powers, rotation, table

PARTITIONS = (("voxel", 8), ("octree", 4, 8), ("kdtree", 8, 6))
SRC = (2.0, 3.5, 1.0)
CHANNELS = {0: 1, 1: 4, 2: 9, 3: 16}


def quad(p0, p1, p2, p3):
    return np.array([p0, p1, p2, p3], np.float64)


def box_quads(lo, hi, turn=0.0):
    """The six faces of the box lo .. hi turned by `turn` radians about the upright axis through its middle, normals outward
    (counter-clockwise seen from outside), and its twelve edges as (a, b, face, face) with the faces numbered 0 .. 5 in the order returned:
    x-, x+, y-, y+, z-, z+.  The edges' ends are the faces' own corners, bit for bit."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    mx, my, cs, sn = 0.5 * (x0 + x1), 0.5 * (y0 + y1), np.cos(turn), np.sin(turn)

    def quad(*pts):
        return np.array([turned(p) for p in pts], np.float64)

    def turned(p):
        return (mx + (p[0] - mx) * cs - (p[1] - my) * sn, my + (p[0] - mx) * sn + (p[1] - my) * cs, p[2]) if turn else tuple(map(float, p))
    f = [quad((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)), quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)),
         quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)), quad((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)),
         quad((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)), quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1))]
    X, Y, Z = (x0, x1), (y0, y1), (z0, z1)
    edges = []
    for i in range(2):
        for k in range(2):
            edges.append((turned((X[0], Y[i], Z[k])), turned((X[1], Y[i], Z[k])), 2 + i, 4 + k))      # along x
            edges.append((turned((X[i], Y[0], Z[k])), turned((X[i], Y[1], Z[k])), 0 + i, 4 + k))      # along y
            edges.append((turned((X[i], Y[k], Z[0])), turned((X[i], Y[k], Z[1])), 0 + i, 2 + k))      # along z
    return np.stack(f), edges


def room(extra):
    m = scenes.shoebox(nface=1)
    verts = np.concatenate([m.verts, extra])
    nverts = np.concatenate([m.nverts, np.full(extra.shape[0], 4, np.int32)])
    return np.ascontiguousarray(verts), np.ascontiguousarray(nverts.astype(np.int32)), m.size


def screen_scene():
    """(verts, nverts, size, ends [3, 2, 3], faces [3, 2]): the top edge and the two upright ones of the screen."""
    v, n, size = room(quad((5, 1.5, 0), (5, 5.5, 0), (5, 5.5, 2.5), (5, 1.5, 2.5))[None])
    ends = np.array([[(5, 1.5, 2.5), (5, 5.5, 2.5)], [(5, 1.5, 0), (5, 1.5, 2.5)], [(5, 5.5, 0), (5, 5.5, 2.5)]], np.float64)
    return v, n, size, ends, np.array([[12, -1]] * 3, np.int32)


def wedge_scene():
    """(verts, nverts, size, ends [12, 2, 3], faces [12, 2]): the box obstacle 4 .. 6 x 2 .. 5 x 0.5 .. 2.5 turned by 0.3 rad, so that an apex
    lies off its faces' planes by a rounding and a leg can meet the edge's second face at a t next to 0."""
    q, edges = box_quads((4.0, 2.0, 0.5), (6.0, 5.0, 2.5), 0.3)
    v, n, size = room(q)
    ends = np.array([[a, b] for a, b, _, _ in edges], np.float64)
    return v, n, size, ends, np.array([[12 + f0, 12 + f1] for _, _, f0, f1 in edges], np.int32)


SCREEN_RCV = [((8.0, 3.5, 1.0), 0.25, "behind the screen"), ((7.0, 3.0, 0.8), 0.2, "behind"), ((7.5, 4.0, 1.2), 0.3, "behind"),
              ((6.0, 3.5, 0.5), 0.2, "behind, close"), ((7.0, 3.5, 3.8), 0.25, "lit over the top"), ((3.0, 1.0, 1.0), 0.25, "lit, the source's side"),
              ((6.0, 0.5, 1.0), 0.2, "lit past the side"), ((8.5, 5.0, 0.6), 0.25, "behind")]
WEDGE_RCV = [((8.0, 3.5, 3.4), 0.25, "behind, above the top"), ((6.5, 5.6, 1.5), 0.2, "behind the y = 5 side"), ((6.5, 1.4, 1.5), 0.2, "behind the y = 2 side"),
             ((8.0, 3.5, 0.2), 0.15, "behind, below the bottom"), ((3.0, 6.0, 1.0), 0.25, "lit"), ((5.0, 6.5, 1.5), 0.25, "lit beside the box"),
             ((7.0, 6.2, 2.0), 0.2, "behind the y = 5 side, high"), ((2.5, 1.0, 3.0), 0.25, "lit")]
WEDGE_SRC = (2.0, 3.5, 1.5)


@dataclasses.dataclass
class DiffractCase:
    name: str
    scene: str                           # "screen", "wedge", or a sweep's own
    partition: tuple
    pos: tuple
    centers: np.ndarray
    radii: np.ndarray
    ends: np.ndarray                     # [E, 2, 3]
    faces: np.ndarray                    # [E, 2]
    inv_lambda: tuple                    # B values
    order: int = 0                       # 0: one channel; 1, 2, 3: directional, 4 / 9 / 16 channels
    R: int = 0
    map: bool = False
    frac_bits: int = 40
    n_bins: int = 64
    bin_len: float = 0.25
    n_weight: int = 4097
    max_detour: float = float("inf")
    mesh: tuple = None                   # (verts, nverts) of a sweep's scene

    @property
    def B(self):
        return len(self.inv_lambda)

    @property
    def K(self):
        return self.centers.shape[0]

    @property
    def shape(self):
        return (self.K, self.n_bins, self.B) + ((CHANNELS[self.order],) if self.order else ())

    def geometry(self):
        if self.mesh is not None:
            return self.mesh
        return (screen_scene() if self.scene == "screen" else wedge_scene())[:2]

    def source(self):
        return (np.array(self.pos, np.float64), powers(self.B), rotation() if self.R else None, self.R, table(self.R, self.B) if self.R else None)


def placed(rows):
    return np.array([r[0] for r in rows], np.float64), np.array([r[1] for r in rows], np.float64)


LAMBDA = {1: (2.9,), 3: (0.36, 2.9, 23.3), 8: tuple(62.5 * 2.0 ** b / 343.0 for b in range(8))}      # f_b / c: octave bands from 62.5 Hz, c = 343 m/s


def screen(name, partition, B, order, **kw):
    _, _, _, ends, faces = screen_scene()
    c, r = placed(SCREEN_RCV)
    a = dict(pos=SRC, centers=c, radii=r, ends=ends, faces=faces, inv_lambda=LAMBDA[B], order=order)
    a.update(kw)
    return DiffractCase(name, "screen", partition, **a)


def map_receivers(K, rows, size, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.06, 0.94, (K, 3)) * np.asarray(size)
    r = rng.uniform(0.1, 0.25, K)
    pc, pr = placed(rows)
    c[:pc.shape[0]], r[:pc.shape[0]] = pc, pr
    return np.ascontiguousarray(c), r


def cases():
    """The fixed cases: the screen at B = 1, 3, 8, one to sixteen channels and the three partitions; the wedge; the numeric edges; the sizes."""
    V, O, T = PARTITIONS
    _, _, size, s_ends, s_faces = screen_scene()
    _, _, _, w_ends, w_faces = wedge_scene()
    wc, wr = placed(WEDGE_RCV)
    out = [screen("screen-B1", V, 1, 0), screen("screen-B3-dir", O, 3, 1, frac_bits=30), screen("screen-B8-dir2", T, 8, 2, n_weight=2 ** 40, frac_bits=20),
           screen("screen-B3-dir3", V, 3, 3, n_weight=1), screen("screen-B8-octree", O, 8, 0), screen("screen-B1-kdtree-dir", T, 1, 1),
           DiffractCase("wedge-B3", "wedge", V, WEDGE_SRC, wc, wr, w_ends, w_faces, LAMBDA[3]),
           DiffractCase("wedge-B1-dir-octree", "wedge", O, WEDGE_SRC, wc, wr, w_ends, w_faces, LAMBDA[1], order=1),
           DiffractCase("wedge-B8-kdtree", "wedge", T, WEDGE_SRC, wc, wr, w_ends, w_faces, LAMBDA[8])]
    # ---- numeric edges, on the screen
    top = s_ends[0]                                                                    # (5, 1.5, 2.5) -> (5, 5.5, 2.5)
    ec, er = placed([((8.0, 1.5, 1.0), 0.25, "tr == 0 with the source at y = 1.5: t == 0"), ((8.0, 3.5, 1.0), 0.25, "an ordinary pair beside it")])
    out.append(DiffractCase("edge-t0", "screen", V, (2.0, 1.5, 1.0), ec, er, top[None], s_faces[:1], LAMBDA[1]))
    ec, er = placed([((8.0, 5.5, 1.0), 0.25, "tr == 1 with the source at y = 5.5: t == 1"), ((8.0, 3.5, 1.0), 0.25, "an ordinary pair")])
    out.append(DiffractCase("edge-t1", "screen", T, (2.0, 5.5, 1.0), ec, er, top[None], s_faces[:1], LAMBDA[1]))
    line = np.array([[(3.0, 3.5, 1.0), (4.0, 3.5, 1.0)]])                               # a free edge on the line through the source and receiver 0
    out.append(DiffractCase("edge-on-line", "screen", T, SRC, *placed([((8.0, 3.5, 1.0), 0.25, "on the edge's line"), ((7.0, 3.0, 0.8), 0.2, "off it")]),
                            np.concatenate([line, s_ends]), np.array([[-1, -1]] + s_faces.tolist(), np.int32), LAMBDA[3]))
    out.append(screen("edge-apex-in-sphere", V, 1, 0, centers=np.array([(5.5, 3.5, 2.0), (8.0, 3.5, 1.0)]), radii=np.array([1.0, 0.25])))
    one = dict(centers=np.array([(8.0, 3.5, 1.0)]), radii=np.array([0.25]), ends=top[None], faces=s_faces[:1])
    delta = float(dr.pairs(SRC, top[None], one["centers"], one["radii"], np.inf)["delta"][0])
    out.append(screen("edge-detour-at-limit", V, 1, 0, max_detour=delta, **one))
    out.append(screen("edge-detour-one-ulp-over", V, 1, 0, max_detour=float(np.nextafter(delta, 0.0)), **one))
    out.append(screen("edge-detour-0", O, 1, 0, max_detour=0.0))
    out.append(screen("edge-detour-1m", T, 3, 1, max_detour=1.0))
    out.append(screen("edge-lambda-0-and-huge", V, 3, 0, inv_lambda=(0.0, 1e300, 1.7976931348623157e308)))
    c, r = placed(SCREEN_RCV)
    c, r = c.copy(), r.copy()
    c[1], r[1] = (2.1, 3.5, 1.0), 0.5
    out.append(screen("edge-source-in-receiver", O, 1, 0, centers=c, radii=r))
    out.append(screen("edge-short-histogram", T, 3, 1, n_bins=26, bin_len=0.25))           # 6.5 m: the longer paths arrive beyond it
    out.append(screen("edge-directivity", V, 3, 1, R=4))
    out.append(screen("edge-frac-62", O, 1, 0, frac_bits=62, n_weight=2 ** 40))
    # ---- sizes: E = 1, 63, 65, 257 by duplicated edges; K = 257 through a receiver map (two tiles)
    for E, part in ((1, V), (63, O), (65, T), (257, V)):
        idx = np.arange(E) % 3
        out.append(screen(f"size-E{E}", part, 1, 0, ends=s_ends[idx], faces=s_faces[idx]))
    mc, mr = map_receivers(257, SCREEN_RCV, size, 5)
    mc[256], mr[256] = (7.2, 3.2, 0.9), 0.2                                            # the second tile's one receiver, in the shadow
    idx = np.arange(65) % 3
    out.append(screen("size-K257-map", V, 3, 0, centers=mc, radii=mr, map=True, n_bins=32, bin_len=0.5))
    out.append(screen("size-K257-map-E65-dir", O, 1, 1, centers=mc, radii=mr, map=True, ends=s_ends[idx], faces=s_faces[idx], n_bins=32, bin_len=0.5))
    assert len({c.name for c in out}) == len(out)
    return out


def case_named(name):
    return next(c for c in cases() if c.name == name)


def sweep_case(seed):
    """A drawn scene: one or two upright screens and, on odd seeds, a box obstacle; every screen's four edges (free) and the box's twelve."""
    rng = np.random.default_rng(1000 + seed)
    extra, ends, faces = [], [], []
    P = 12
    for _ in range(int(rng.integers(1, 3))):
        x, y0 = rng.uniform(3.0, 7.0), rng.uniform(0.5, 3.0)
        y1, z1, dx = y0 + rng.uniform(1.5, 3.5), rng.uniform(1.5, 3.5), rng.uniform(-1.0, 1.0)
        p = [(x, y0, 0.0), (x + dx, y1, 0.0), (x + dx, y1, z1), (x, y0, z1)]
        extra.append(quad(*p))
        for i in range(4):
            ends.append((p[i], p[(i + 1) % 4]))
            faces.append((P, -1))
        P += 1
    if seed % 2:
        lo = rng.uniform((2.0, 1.0, 0.0), (6.0, 4.0, 1.0))
        hi = lo + rng.uniform(0.5, 2.0, 3)
        q, edges = box_quads(tuple(lo), tuple(hi), float(rng.uniform(0.0, 1.5)))
        extra += list(q)
        ends += [(a, b) for a, b, _, _ in edges]
        faces += [(P + f0, P + f1) for _, _, f0, f1 in edges]
    v, n, size = room(np.stack(extra))
    K = int(rng.integers(1, 13))
    c = rng.uniform(0.06, 0.94, (K, 3)) * np.asarray(size)
    r = rng.uniform(0.1, 0.3, K)
    B = (1, 3, 8)[seed % 3]
    lam = tuple(rng.uniform(0.1, 30.0, B))
    return DiffractCase(f"sweep-{seed}", "sweep", PARTITIONS[(seed // 3) % 3], tuple(rng.uniform(0.1, 0.9, 3) * np.asarray(size)), np.ascontiguousarray(c), r,
                        np.array(ends, np.float64), np.array(faces, np.int32), lam, order=(seed // 2) % 4, R=4 if seed % 5 == 0 else 0,
                        frac_bits=(40, 20, 62)[seed % 3], n_bins=(64, 40)[seed % 2], n_weight=(4097, 1, 2 ** 40)[(seed // 4) % 3],
                        max_detour=(float("inf"), 2.0)[(seed // 7) % 2], mesh=(v, n))


SWEEP = range(50)
_ORACLES, _KEPT = {}, {}


def oracle_of(case):
    """The oracle partition of the case's scene; kept for the fixed scenes."""
    key = (case.scene, case.partition) if case.mesh is None else None
    if key in _ORACLES:
        return _ORACLES[key]
    verts, nverts = case.geometry()
    To = po.Topology(verts, nverts)
    kind, *par = case.partition
    o = po.VoxelGrid([To], domain=par[0]) if kind == "voxel" else (po.Octree if kind == "octree" else po.KDTree)([To], *par)
    if key is not None:
        _ORACLES[key] = o
    return o


def _run(case, hist, det, seen, second_word=True):
    return dr.diffract(oracle_of(case), *case.source(), case.ends, case.faces, case.inv_lambda, case.centers, case.radii, case.n_weight, case.n_bins,
                       case.bin_len, case.frac_bits, case.max_detour, hist, det, seen, None, 16, second_word)


def reference(case, second_word=True):
    """diffract() of a case onto zeros at the case's order: dict of hist, det, pairs (the count) and seen.  Kept and served again: the
    tests share it and leave it unchanged."""
    key = (case.name, second_word)
    if key in _KEPT:
        return _KEPT[key]
    seen = {}
    det = np.zeros((case.K, 2), np.uint64)

    def run():
        hist = np.zeros(case.shape[:3] + ((4,) if case.order else ()), np.uint64)
        return hist, _run(case, hist, det, seen, second_word)
    hist, m = ambi_ref.run(case.order, run) if case.order > 1 else run()
    out = dict(hist=hist, det=det, pairs=m, seen=seen)
    if len(_KEPT) < 96:
        _KEPT[key] = out
    return out


def digest(ref):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(ref["hist"]).tobytes())
    h.update(np.ascontiguousarray(ref["det"]).tobytes())
    h.update(str(int(ref["pairs"])).encode())
    return h.hexdigest()
