"""Inputs for the partition builders' device tests (hare_amd/csrc/build_gpu.cpp, build_kernels.hip: gpu_build_voxel_fixed,
gpu_build_voxel_adaptive, gpu_build_octree): case records built from numpy and the oracle alone, no GPU.  BuildCase is the one record: an
id, the topologies, the builder -- ("fixed", D), ("adaptive", max_domain, avg_polys) or ("octree", max_depth, max_polys) -- and what the
case claims to reach (`reaches`), which tests/test_build_cases.py counts again on the reference.  reference(case) is oracle.pyoracle's
VoxelGrid (the literal D^3 x P loop, build_mode 0, where D^3 x P < 3e7; the polygon-major restatement otherwise) or Octree(...).export(),
as tests/test_host_builders.py uses them.  The contract is identity: the order of a list decides who wins an exact-t tie.

Two sets.  edge_cases(): fixed and named, each at a size where the device builders take another path -- the three list classes of the
fixed grid's sort (n <= 48 insertion sort, 49 .. 8192 bitonic in LDS, > 8192 ordered fill), the scan's recursion steps (2048 counters a
block: one level up to D = 12, two up to D = 161, three from D = 162), the occupancy layouts (D = 80 / 81, 160 / 161), the adaptive
grid's stop rule, the octree's 8192-entry segments and 256-entry ballot rounds.  sweep_case(seed): one scene of degenerate geometry and a
builder drawn from a seed (tools/fuzz_builders.py runs them over any range).  build(case) builds the product's partition, compare(...)
names the first differing cell or node.  digest(reference) is the SHA-256 that tests/golden/build_reference_digests.json pins."""
import dataclasses
import functools
import hashlib
import json
import os

import numpy as np

import hare_amd as H
from hare_amd import capi
from oracle import pyoracle as po

SMALL_MAX = 48           # build_gpu.cpp: longest list hare_vb_sort_small sorts itself
BIG_LIST = 8192          # build_kernels.hip kBigList: longest list the LDS sorter takes; longer ones are filled in order
SEG = 8192               # build_gpu.cpp kSeg: parent-list entries per octree task
SCAN_BLOCK = 2048        # counters per block of scan_u32
LENGTHS = (0, 1, 2, 47, 48, 49, 50, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 8194)
SWEEP_DOMAINS = (1, 2, 3, 7, 12, 13, 31, 40)
OCT_ENTRIES_MAX = 400_000        # a sweep octree's estimated list entries (P x 8 per level whose nodes are under 1 m): the depth is cut to it


@dataclasses.dataclass
class BuildCase:
    name: str
    topos: tuple                         # ((verts [P, 4, 3], nverts [P]), ...)
    builder: tuple
    reaches: dict = dataclasses.field(default_factory=dict)
    why: str = ""
    shoot: bool = False                  # the device test also shoots rays through the grid
    aim: np.ndarray = None               # [n, 3] points that half of those rays are aimed at (the clusters)

    @property
    def kind(self):
        return "octree" if self.builder[0] == "octree" else "voxel"

    @property
    def P(self):
        return sum(v.shape[0] for v, _ in self.topos)

    def describe(self):
        return f"{self.name}: {' '.join(str(x) for x in self.builder)}, topologies of {[v.shape[0] for v, _ in self.topos]} polygons"


# ---- the reference and the product
_KEPT = {}


def reference(case, keep=False):
    """What the builders must return.  A grid: dict(ct, char_step, obox_min, obox_max, voxel_dims, lists [(start, items) per topology],
    total_items); a tree: dict(nodes = (boxes, first_child, item_start, item_count, items)).  `oracle` is the oracle's object (for shoots),
    `topos` its topologies.  keep: served again under the case's name (the fixed set, whose tests share it and leave it unchanged)."""
    if keep and case.name in _KEPT:
        return _KEPT[case.name]
    To = [po.Topology(v, nv) for v, nv in case.topos]
    b = case.builder
    if b[0] == "octree":
        o = po.Octree(To, b[1], b[2])
        out = dict(nodes=o.export())
    else:
        if b[0] == "fixed":
            o = po.VoxelGrid(To, domain=b[1], build_mode=0 if b[1] ** 3 * case.P < 3e7 else 1)
        else:
            o = po.VoxelGrid(To, max_domain=b[1], avg_polys=b[2])
        lists = [o.lists(m) for m in range(len(To))]
        out = dict(ct=o.ct, char_step=o.char_step, obox_min=o.obox_min, obox_max=o.obox_max, voxel_dims=o.voxel_dims, lists=lists,
                   total_items=int(lists[0][0][-1]))
    out.update(oracle=o, topos=To)
    if keep:
        _KEPT[case.name] = out
    return out


def digest(ref):
    h = hashlib.sha256()
    arrays = list(ref["nodes"]) if "nodes" in ref else [np.array([ref["ct"]], np.int64), np.array([ref["char_step"]]), ref["obox_min"], ref["obox_max"],
                                                         ref["voxel_dims"]] + [a for pair in ref["lists"] for a in pair]
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str} {a.shape}\n".encode())
        h.update(a.tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def pinned_digests():
    """tests/golden/build_reference_digests.json: digest() of every edge case ("edge/" + name) and of the sweep's seeds ("sweep/" 0 .. N - 1)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "build_reference_digests.json")) as f:
        return json.load(f)


def rebuild(part, builder):
    """The builder's C call on a scene that exists (a second call replaces the partition the scene holds)."""
    if builder[0] == "octree":
        capi.check(capi.lib.hare_octree_build(part._h, int(builder[1]), int(builder[2])))
        return part
    if builder[0] == "fixed":
        capi.check(capi.lib.hare_voxel_build(part._h, int(builder[1])))
    else:
        capi.check(capi.lib.hare_voxel_build_adaptive(part._h, int(builder[1]), int(builder[2])))
    info = part.info()
    part.Char_Step, part.VoxelCt = info.char_step, info.ct
    return part


def build(case, host=False):
    """The product's partition of the case; host: scene option "build_host" set before the build (the host builders)."""
    cls = H.Octree if case.kind == "octree" else H.Voxel_Grid
    part = cls.__new__(cls)
    H.Spatial_Partition.__init__(part, [H.Topology(v, nv) for v, nv in case.topos])
    if host:
        part.set_option("build_host", 1)
    return rebuild(part, case.builder)


def first_difference(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"{what}: shape {got.shape}, wanted {want.shape}"
    if np.array_equal(got, want):
        return None
    i = np.argwhere(np.atleast_1d(got != want))[0]
    return f"{what} differs first at {i.tolist()}: {np.atleast_1d(got)[tuple(i)]!r}, wanted {np.atleast_1d(want)[tuple(i)]!r}"


def compare(case, part, ref):
    """None, or the first difference between the product's partition and the reference: the cell (its list printed both ways) or the node."""
    if case.kind == "octree":
        for a, b, what in zip(part.nodes(), ref["nodes"], ("boxes", "first_child", "item_start", "item_count", "items")):
            bad = first_difference(a, b, "node " + what)
            if bad:
                return bad
        info = part.info()
        if (info.n_nodes, int(info.total_items)) != (len(ref["nodes"][1]), len(ref["nodes"][4])):
            return f"info: {info.n_nodes} nodes, {info.total_items} items"
        return None
    info = part.info()
    for what, got, want in (("ct", info.ct, ref["ct"]), ("VoxelCt", part.VoxelCt, ref["ct"]), ("n_topos", info.n_topos, len(case.topos)),
                            ("char_step", info.char_step, ref["char_step"]), ("Char_Step", part.Char_Step, ref["char_step"]),
                            ("total_items", int(info.total_items), ref["total_items"]), ("obox_min", tuple(info.obox_min), tuple(ref["obox_min"])),
                            ("obox_max", tuple(info.obox_max), tuple(ref["obox_max"])), ("voxel_dims", tuple(info.voxel_dims), tuple(ref["voxel_dims"])),
                            ("box_dims", tuple(info.box_dims), tuple(ref["obox_max"] - ref["obox_min"]))):
        if got != want:
            return f"{what}: {got!r}, wanted {want!r}"
    for m, (so, io) in enumerate(ref["lists"]):
        s, i = part.Voxel_Inv(m)
        if np.array_equal(s, so) and np.array_equal(i, io):
            continue
        if s.shape != so.shape:
            return f"topology {m}: {s.shape[0] - 1} cells, wanted {so.shape[0] - 1}"
        n, no = np.diff(s.astype(np.int64)), np.diff(so.astype(np.int64))
        for c in range(len(n)):
            a, b = i[s[c]:s[c] + n[c]], io[so[c]:so[c] + no[c]]
            if n[c] != no[c] or not np.array_equal(a, b):
                k = 0 if n[c] != no[c] else int(np.nonzero(a != b)[0][0])
                return (f"topology {m} cell {c} (x {c // ref['ct'] ** 2}, y {c // ref['ct'] % ref['ct']}, z {c % ref['ct']}): {n[c]} entries, wanted {no[c]}; "
                        f"from entry {k}: {a[k:k + 6].tolist()}, wanted {b[k:k + 6].tolist()}")
        return first_difference(s, so, f"topology {m} starts")
    return None


def check_case(case, ref, host=False):
    """One case as the sweep runs it: built (host: with the host builders), `built_on_device` as expected, compare(), a second build equal to
    the first byte for byte, and for a grid one shoot per topology against the oracle's events.  None, or what differs."""
    part = build(case, host)
    on_device = 0 if host or (case.kind == "octree" and len(case.topos) > 1) else 1
    if part.info().built_on_device != on_device:
        return f"built_on_device {part.info().built_on_device}, wanted {on_device}"
    bad = compare(case, part, ref)
    if bad:
        return bad
    again = build(case, host)
    if case.kind == "octree":
        same = all(a.tobytes() == b.tobytes() for a, b in zip(part.nodes(), again.nodes()))
    else:
        same = all(a.tobytes() == b.tobytes() for m in range(len(case.topos)) for a, b in zip(part.Voxel_Inv(m), again.Voxel_Inv(m)))
    if not same:
        return "a second build differs from the first"
    if case.kind == "voxel" and case.shoot and not host:
        rays = rays_for(case, 2000)
        for top in range(len(case.topos)):
            want, _ = ref["oracle"].shoot(rays, top, nthreads=16)
            got, _ = part.Shoot_batch(rays, top)
            for f in ("hit", "poly_id", "t", "u", "v", "x", "y", "z"):
                if not np.array_equal(got[f], want[f]):
                    return f"shoot, topology {top}: X_Event.{f} differs first at ray {int(np.nonzero(got[f] != want[f])[0][0])}"
    return None


def rays_for(case, n=4000, seed=5):
    """n rays [n, 6] for a grid case: origins in and around the bounds; half of the directions towards the case's `aim` points (polygon
    centroids where it names none), so that the long lists are scanned, the others drawn."""
    rng = np.random.default_rng(seed)
    v, nv = case.topos[-1]
    lo = np.min([t[0][:, :3].reshape(-1, 3).min(axis=0) for t in case.topos], axis=0)
    hi = np.max([t[0][:, :3].reshape(-1, 3).max(axis=0) for t in case.topos], axis=0)
    o = rng.uniform(-0.2, 1.2, (n, 3)) * (hi - lo) + lo
    d = rng.normal(size=(n, 3))
    aim = v[:, :3].mean(axis=1) if case.aim is None else case.aim
    k = n // 2
    d[:k] = aim[rng.integers(0, len(aim), k)] + rng.normal(0, 0.01, (k, 3)) * (hi - lo) - o[:k]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[3::101, 1] = 0.0                                                   # some axis-parallel components
    return np.ascontiguousarray(np.concatenate([o, d], axis=1))


# ---- scenes
def as_topology(tris, quad=None):
    """[P, 3, 3] triangles -> (verts [P, 4, 3], nverts); quad [P] bool: those become the exact parallelogram v0, v1, v2, v0 + (v2 - v1)."""
    tris = np.asarray(tris, np.float64)
    P = tris.shape[0]
    verts, nverts = np.zeros((P, 4, 3)), np.full(P, 3, np.int32)
    verts[:, :3] = tris
    if quad is not None and quad.any():
        verts[quad, 3] = verts[quad, 0] + (verts[quad, 2] - verts[quad, 1])
        nverts[quad] = 4
    return np.ascontiguousarray(verts), nverts


def corner_triangles(lo, hi):
    """Two small triangles that fix a topology's bounds at the cube [lo, hi]^3."""
    e = (hi - lo) / 32.0
    return [np.array([[lo, lo, lo], [lo + e, lo, lo], [lo, lo + e, lo]], float), np.array([[hi, hi, hi], [hi - e, hi, hi], [hi, hi - e, hi]], float)]


def tiny_triangles(rng, center, n, vd):
    """n triangles of edge vd / 16 around `center`, offset by multiples of vd / 64, at most vd / 8: far from every padded face of a cell
    of width vd that `center` is the middle of."""
    p = center + rng.integers(-8, 9, (n, 3)) / 64.0 * vd
    return np.stack([p, p + [vd / 16, 0, 0], p + [0, vd / 16, 0]], axis=1)


def exact_lengths(lengths=LENGTHS, D=4, seed=0, quads=0.0, split=None):
    """Cell k of the D^3 grid over an 8 m cube (the two corner cells left out: they hold the corner triangles) gets lengths[k] tiny
    triangles about its centre; the polygon order is permuted, so that no cell's list is a contiguous index range.  quads: that share become
    parallelograms.  split: lists of at least that length go to a second topology (both carry the corner triangles, so both span the cube).
    Returns (topologies, the clusters' centres)."""
    rng = np.random.default_rng(seed)
    L = 8.0
    vd = L / D
    cells = [(x, y, z) for x in range(D) for y in range(D) for z in range(D)]
    cells = [c for c in cells if c not in ((0, 0, 0), (D - 1, D - 1, D - 1))][:len(lengths)]
    assert len(cells) == len(lengths)
    parts = [corner_triangles(0.0, L), corner_triangles(0.0, L)]
    centres = []
    for c, n in zip(cells, lengths):
        ctr = (np.array(c) + 0.5) * vd
        if n:
            centres.append(ctr)
        parts[1 if split is not None and n >= split else 0].extend(tiny_triangles(rng, ctr, n, vd))
    topos = []
    for tris in parts[:2 if split is not None else 1]:
        tris = np.array(tris)
        tris = tris[rng.permutation(len(tris))]
        topos.append(as_topology(tris, rng.random(len(tris)) < quads))
    return tuple(topos), np.array(centres)


def scattered(P, seed, lo=0.0, hi=8.0, big=2):
    """P polygons in the cube [lo, hi]^3: the two corner triangles (the far one falls in the grid's last cell), `big` polygons across half
    the cube, the rest small, every fourth a parallelogram; dyadic coordinates."""
    rng = np.random.default_rng(seed)
    L = hi - lo
    n = P - 2
    c = lo + rng.integers(8, 248, (n, 3)) / 256.0 * L
    e1 = rng.integers(-6, 7, (n, 3)) / 256.0 * L
    e2 = rng.integers(-6, 7, (n, 3)) / 256.0 * L
    e1[:big] *= 20
    e2[:big] *= 20
    tris = np.clip(np.stack([c, c + e1, c + e1 + e2], axis=1), lo, hi)
    quad = np.concatenate([[False, False], np.arange(n) % 4 == 3])
    quad[2:2 + big] = False                                              # the clipped ones stay triangles
    tris = np.concatenate([np.array(corner_triangles(lo, hi)), tris])
    perm = rng.permutation(P)
    perm = np.concatenate([perm[perm != 1], [1]])                        # the far corner's triangle is the last polygon as well
    return as_topology(tris[perm], quad[perm])


def octants(counts, seed, lo=-8.0, hi=0.0, quads=0.0):
    """A model in [lo, 0]^3 with hi = 0: there the root cube, centred at max + min / 2 as the reference writes it, is centred on the model,
    so the root's eight children are the model's octants.  counts[i] polygons fall in child i alone (bit 4: x, 2: y, 1: z high), in a
    cluster about the octant's middle, well clear of the children's padded planes; the two corner triangles count towards octants 0 and 7."""
    assert hi == 0.0 and len(counts) == 8 and counts[0] >= 1 and counts[7] >= 1
    rng = np.random.default_rng(seed)
    L = hi - lo
    tris = corner_triangles(lo, hi)
    for i, n in enumerate(counts):
        ctr = np.array([lo + L * (0.75 if i & b else 0.25) for b in (4, 2, 1)])
        tris.extend(tiny_triangles(rng, ctr, n - (i in (0, 7)), L / 4))
    tris = np.array(tris)
    tris = tris[rng.permutation(len(tris))]
    return as_topology(tris, rng.random(len(tris)) < quads)


def spread(P, seed):
    """P polygons for a root list of exactly P entries: the eight octants of octants() filled as evenly as P allows."""
    return octants([P // 8 + (i < P % 8) for i in range(8)], seed)


def exact_mean(m, seed=0, two=False):
    """A scene whose non-empty cells at ct = 8 all hold exactly m polygons, so that the mean list length there is the integer m.  two: two
    topologies whose cells hold m - 1 and m + 1, as many non-empty cells each: only the mean over both is m."""
    rng = np.random.default_rng(seed)
    vd = 1.0
    cells = [(1, 1, 1), (2, 5, 3), (6, 2, 4), (3, 3, 6), (5, 6, 1), (4, 1, 5)]
    topos = []
    for per in ((m - 1, m + 1) if two else (m,)):
        tris = []
        for j, corner in enumerate(corner_triangles(0.0, 8.0)):          # each corner cell: its corner triangle and per - 1 more next to it
            tris.append(corner)
            tris.extend(tiny_triangles(rng, np.full(3, 0.5 if j == 0 else 7.5), per - 1, vd))
        for c in cells:
            tris.extend(tiny_triangles(rng, np.array(c) + 0.5, per, vd))
        tris = np.array(tris)
        topos.append(as_topology(tris[rng.permutation(len(tris))]))
    return tuple(topos)


def grid_planes(lo, hi, D):
    """The cell planes of a D-grid over a topology bounded by [lo, hi] per axis, as build_host.cpp's voxel_grid_bounds and hare_math.h's
    voxel_lo / voxel_hi form them: (planes k vd + omin, padded low faces, padded high faces), each [3, D - 1]."""
    omin = (((lo - 0.000000000001) - 0.001) - 0.1)                       # Finish_Topology's 1e-12, then the grid's two margins
    omax = (((hi + 0.000000000001) + 0.001) + 0.1)
    vd = (omax - omin) / D
    k = np.arange(1, D)[None, :]
    return k * vd[:, None] + omin[:, None], (k * vd[:, None] - 0.001) + omin[:, None], (k * vd[:, None] + 0.001) + omin[:, None]


def degenerate(rng, P, D, scale=1.0, offset=0.0, quads=0.25):
    """P polygons of the degenerate mix in the cube [offset, offset + 10 scale]^3, which the two corner triangles span: small and large
    polygons, slivers, zero-area (collinear) and repeated-vertex polygons, polygons with one corner or all corners exactly on a plane of the
    D-grid, polygons lying exactly in a padded face (plane -+ 0.001, where neighbouring cells' boxes touch), two polygons across the whole
    grid.  Every corner is clipped to the cube, so the bounds, and with them the planes, are the corner triangles'."""
    lo, hi = offset, offset + 10.0 * scale
    n = P - 2
    c = rng.uniform(lo, hi, (n, 3))
    e1 = rng.normal(0, 0.5 * scale, (n, 3))
    e2 = rng.normal(0, 0.5 * scale, (n, 3))
    cls = rng.choice(8, n, p=[0.52, 0.04, 0.08, 0.06, 0.06, 0.08, 0.08, 0.08])
    e1[cls == 1] *= 8                                                    # large
    e2[cls == 1] *= 8
    sl = cls == 2                                                        # slivers
    e2[sl] = e1[sl] + rng.normal(0, 1e-4 * scale, (int(sl.sum()), 3))
    e2[cls == 3] = e1[cls == 3] * 0.5                                    # zero area: v2 on the line v0 v1 (to rounding)
    tris = np.stack([c, c + e1, c + e1 + e2], axis=1)
    rep = cls == 4                                                       # a repeated corner
    tris[rep, 2] = tris[rep, 1]
    tris[:2] = [[[lo] * 3, [hi] * 3, [lo, hi, lo]], [[hi, lo, lo], [lo, hi, hi], [hi, hi, lo]]]        # across the whole grid
    tris = np.clip(tris, lo, hi)
    if D > 1:
        planes, low, high = grid_planes(np.full(3, lo), np.full(3, hi), D)
        for j in np.nonzero(cls >= 5)[0]:
            a, k = int(rng.integers(0, 3)), int(rng.integers(0, D - 1))
            if cls[j] == 5:                                              # one corner on a cell plane
                tris[j, int(rng.integers(0, 3)), a] = planes[a, k]
            else:                                                        # the polygon in a cell plane / in a padded face
                tris[j, :, a] = planes[a, k] if cls[j] == 6 else (low if rng.random() < 0.5 else high)[a, k]
    v3 = tris[:, 0] + (tris[:, 2] - tris[:, 1])                          # a parallelogram only where its fourth corner stays in the cube
    quad = np.concatenate([[False, False], (rng.random(n) < quads) & np.isin(cls, (0, 1, 6, 7)) & ((v3 >= lo) & (v3 <= hi)).all(axis=1)])
    quad[2:4] = False
    tris = np.concatenate([np.array(corner_triangles(lo, hi)), tris])
    perm = rng.permutation(P)
    return as_topology(tris[perm], quad[perm])


# ---- edge cases
def fixed_cases():
    out = []
    t, aim = exact_lengths()
    why = "lists of 0 .. 8194 entries in one grid: insertion sort, LDS sort and ordered fill side by side"
    out.append(BuildCase("lengths-D4", t, ("fixed", 4), dict(lengths=LENGTHS, P=46217), why, shoot=True, aim=aim))
    t, aim = exact_lengths(seed=1, quads=0.25)
    out.append(BuildCase("lengths-D4-quads", t, ("fixed", 4), dict(lengths=LENGTHS, P=46217, quads=True), why + ", a quarter parallelograms", aim=aim))
    t, aim = exact_lengths(seed=2, split=4095)
    out.append(BuildCase("lengths-D4-two-topologies", t, ("fixed", 4), dict(lengths=LENGTHS, long_in=1), why + ", the long lists in topology 1", aim=aim))
    for D in (12, 13, 80, 81, 160, 161, 162):                            # a cube of 32 m: a cell is wider than the grid's 0.101 m margin, so the corner triangles
                                                                         # fall in the first and the last cell, the first and the last block of counters
        levels = 1 if D ** 3 + 1 <= SCAN_BLOCK else 2 if D ** 3 + 1 <= SCAN_BLOCK ** 2 else 3
        out.append(BuildCase(f"scan-D{D}", (scattered(300, 100 + D, hi=32.0),), ("fixed", D), dict(scan_levels=levels, first_and_last_block=True),
                             f"{D ** 3 + 1} counters: {levels} scan level(s); occupancy layout of D = {D}", shoot=D >= 80))
    t = (degenerate(np.random.default_rng(31), 600, 7), degenerate(np.random.default_rng(32), 200, 7))
    out.append(BuildCase("degenerate-D7", t, ("fixed", 7), dict(on_planes=True), "the degenerate mix on the planes of its own grid, two topologies", shoot=True))
    out.append(BuildCase("degenerate-D13-far", (degenerate(np.random.default_rng(33), 900, 13, scale=1e3, offset=-512e3),), ("fixed", 13), dict(on_planes=True),
                         "the degenerate mix at 10 km, 512 km from the origin", shoot=True))
    out.append(BuildCase("degenerate-D3-mm", (degenerate(np.random.default_rng(34), 500, 3, scale=1e-3),), ("fixed", 3), dict(),
                         "a model of 1 cm: the 0.1 m margin is most of the grid"))
    return out


def adaptive_cases():
    """The stop rule `k > 1 && sum / cnt < avg_polys` (levels k = 0, 1, 2, ... give ct = 2, 4, 8, ...): it cannot fire before ct = 8; with
    avg_polys 0 or 1 it never fires (a mean over non-empty cells is at least 1); with 10^6 it fires at ct = 8."""
    out = []
    one = (scattered(240, 7),)
    two = (scattered(240, 7), scattered(90, 8))
    for tag, t in (("one", one), ("two", two)):
        for md in (1, 2, 3, 5):
            for avg in (0, 1, 10 ** 6):
                ct = 2 ** md if avg <= 1 else min(2 ** md, 8)
                out.append(BuildCase(f"adaptive-{tag}-md{md}-avg{avg}", t, ("adaptive", md, avg), dict(ct=ct), "the stop rule's reach", shoot=(md, avg) == (5, 1)))
    m = 3
    for tag, t in (("one", exact_mean(m)), ("two", exact_mean(m, 1, two=True))):
        out.append(BuildCase(f"adaptive-mean-{tag}-equal", t, ("adaptive", 4, m), dict(ct=16, mean8=m), "a mean equal to avg_polys does not stop"))
        out.append(BuildCase(f"adaptive-mean-{tag}-above", t, ("adaptive", 4, m + 1), dict(ct=8, mean8=m), "a mean one under avg_polys stops at ct = 8"))
    return out


def octree_cases():
    out = []
    for P in (8191, 8192, 8193, 16384, 16385):
        depth = 2 if P == 16385 else 1
        out.append(BuildCase(f"octree-root-{P}", (spread(P, P),), ("octree", depth, 1000), dict(parent_counts=(P,)),
                             f"a root list of {P} entries: segments of 8192 full, one short, one over"))
    clusters = (octants([255, 256, 257, 100, 100, 100, 100, 100], 41, quads=0.25),)
    out.append(BuildCase("octree-clusters", clusters, ("octree", 1, 100), dict(leaf_counts=(255, 256, 257), n_nodes=9),
                         "255 / 256 / 257 survivors of a segment, all in one child"))
    out.append(BuildCase("octree-siblings", clusters, ("octree", 2, 256), dict(leaf_counts=(255, 256), split_counts=(257,), n_nodes=17),
                         "siblings of max_polys (a leaf) and max_polys + 1 (splits)"))
    out.append(BuildCase("octree-idle-level", clusters, ("octree", 6, 300), dict(leaf_counts=(255, 256, 257), n_nodes=9),
                         "the second level splits nothing: the build ends under max_depth"))
    out.append(BuildCase("octree-depth0", clusters, ("octree", 0, 4), dict(n_nodes=1), "max_depth 0: the root is the tree"))
    out.append(BuildCase("octree-depth1", (scattered(500, 43, lo=-8.0, hi=0.0),), ("octree", 1, 4), dict(n_nodes=9), "max_depth 1"))
    t, _ = exact_lengths(seed=3)
    out.append(BuildCase("octree-lengths", t, ("octree", 3, 8192), dict(leaf_counts=(4095, 4096, 4097, 8191, 8192, 8193, 8194), parent_min=16385),
                         "parent lists beyond two segments, in permuted order, and leaves of 4095 .. 8194"))
    out.append(BuildCase("octree-degenerate", (degenerate(np.random.default_rng(35), 1500, 8),), ("octree", 4, 20), dict(), "the degenerate mix in a tree"))
    out.append(BuildCase("octree-two-topologies", (scattered(400, 44, lo=-8.0, hi=0.0), scattered(150, 45, lo=-8.0, hi=0.0)), ("octree", 3, 16), dict(host=True),
                         "several topologies: the host builder"))
    return out


@functools.lru_cache(maxsize=None)
def edge_cases():
    out = fixed_cases() + adaptive_cases() + octree_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


# ---- sweep cases
def sweep_case(seed):
    """One case from the seed: the degenerate mix at a scale of 10^-3 .. 10^3, sometimes far from the origin, P = 40 .. 3000, one or two
    topologies, and a builder.  Nothing is redrawn; an octree's depth is cut to OCT_ENTRIES_MAX, and six in ten of the octrees get a model
    that ends at the origin, which the root cube covers (elsewhere the root, centred at max + min / 2, misses most of the model)."""
    rng = np.random.default_rng(0xB17D0000 + int(seed))
    scale = float(10.0 ** rng.integers(-3, 4))
    offset = float(rng.choice([0.0, 0.0, 37.5, -512.0, 1.0e4])) * scale
    P = int(np.exp(rng.uniform(np.log(40.0), np.log(3000.0))))
    which = ("fixed", "adaptive", "octree")[int(rng.integers(0, 3))]
    if which == "fixed":
        builder = ("fixed", int(rng.choice(SWEEP_DOMAINS)))
        D = builder[1]
    elif which == "adaptive":
        builder = ("adaptive", int(rng.integers(1, 6)), int(rng.choice([0, 1, 2, 4, 8, 10 ** 6])))
        D = 8
    else:
        depth, size = int(rng.integers(0, 8)), 20.0 * scale               # the root cube's edge is twice the model's
        while depth > 0 and P * 8 ** sum(size / 2 ** d < 1.0 for d in range(1, depth + 1)) > OCT_ENTRIES_MAX:
            depth -= 1
        builder = ("octree", depth, int(rng.integers(1, 40)))
        D = 8
        if rng.random() < 0.6:                                           # a model that ends at the origin: the root cube covers it (octants())
            offset = -10.0 * scale
    two = bool(rng.random() < (0.15 if which == "octree" else 0.4))      # an octree of several topologies is the host builder's
    topos = [degenerate(rng, P, D, scale, offset)]
    if two:
        topos.append(degenerate(rng, max(40, P // 3), D, scale, offset))
    return BuildCase(f"sweep-{seed}", tuple(topos), builder, why=f"scale {scale:g} offset {offset:g}", shoot=which != "octree")
