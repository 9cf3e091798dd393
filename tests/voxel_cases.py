"""The cases of the tests of the voxel kernels' switches and call modes (tests/test_voxel_cases.py on the oracle alone,
tests/test_gpu_voxel_matrix.py on the device): a case type, a covering array of strength 2 over scene x grid x rays x n x mode x the
thirteen scene options -- every pair of levels of every two factors in at least one case, except the pairs IMPOSSIBLE declares --
generated greedily from one seed, a few fixed cases behind it that put a case into every cell of the voxel kernel table (family x
bitmap x polygons: three factors, which pairs do not promise), and the inputs and the oracle's answer of every case, computed once per
distinct (scene, grid, rays, n, kind of reference) and shared by the option settings.  No GPU, no torch.

Levels that are not the issue's wording, and why:
  * grid: the bitmap is a bit per voxel up to 80 voxels a side, per 2^3 block from 81, per 4^3 block from 161 (scene.h: occ_layout; the
    boundaries are restated and checked in tests/test_voxel_cases.py), so 81 and 161 are the first grids of their kind;
  * ticket_rays: hare_scene_set_option takes 0 ... 4096 and the launcher raises anything below 8 to 8 (launch.cpp: clamp_ticket): 8 is the
    smallest value that reaches a kernel as it was set; 65 is one above a wave;
  * k1p_static_rays 8: K1q's step and floor (K1p raises it to its own floor, 32).
What a mode needs from its rays is put there, so that the reference has something to decide whatever the generator (checked from the
oracle alone in tests/test_voxel_cases.py): a write-back case has every fourth origin pushed out of the grid against its direction
(tie_rays and face_rays start inside); a bounce case has every fourth ray leave the scene at once (the tie scene is a closed box: nothing
would ever retire); an exclusion case and a t_max case have two rays of five turned towards a polygon (random rays into an
open soup hit rarely); a case of ONE ray takes the generator's first ray the plain cast hits."""
import os
import re
import zlib
from functools import lru_cache

import numpy as np

from oracle import pyoracle as po
from tests.helpers import oracle_bounce_loop, soup, soup_rays
from tests.test_gpu_parity import degenerate_rays
from tests.test_gpu_round6 import awkward_rays
from tests.test_gpu_tight import face_rays
from tests.test_gpu_ties import tie_rays, tie_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DEVICE_H = open(os.path.join(ROOT, "hare_amd", "csrc", "hare_device.h")).read()
WINDOW = int(re.search(r"constexpr int kOrderWindow = (\d+);", _DEVICE_H).group(1))       # the order pass's window (order_kernels.hip)
WAVE = 64
MAX_CASES, MAX_RAYS = 150, 8193
BOUNCES = 3
SEED = 20240521

FACTORS = {
    "scene": ("tie", "soup", "two"),
    "grid": ("D1", "D8", "D33", "D81", "D161", "A7"),            # A7: the adaptive grid Voxel_Grid([T], 7, 12)
    "rays": ("tie", "face", "awkward", "degenerate", "soup"),
    "n": (1, WAVE - 1, WAVE, WAVE + 1, WINDOW - 1, WINDOW + 1, 2 * WINDOW + 1),
    "mode": ("closest", "excl", "writeback", "slim", "retired", "occl", "occl_tmax", "own", "bounce"),
    "voxel_kernel": (2, 1),
    "voxel_walk": (1, 0),
    "voxel_overlap": (0, 1),
    "voxel_skip": (0, 1),
    "voxel_tight": (1, 0),
    "wide_drain": (1, 0),
    "coop_tail": (1, 0),
    "voxel_order": (0, 2),
    "ticket_rays": (0, 8, WAVE + 1),
    "k1p_static_rays": (0, 8),
    "batch_chunks": (0, 3),
    "bounce_fused": (0, 1),
    "bounce_pack": (1, 0),
}
NAMES = tuple(FACTORS)
OPTIONS = NAMES[5:]
# what hare_scene_create leaves in a scene: a case puts every option back to these
DEFAULTS = {"voxel_kernel": 0, "voxel_walk": 1, "voxel_overlap": 0, "voxel_skip": 0, "voxel_tight": 1, "wide_drain": 1, "coop_tail": 1,
            "voxel_order": 1, "ticket_rays": 0, "k1p_static_rays": 0, "batch_chunks": 0, "bounce_fused": 0, "bounce_pack": 1}
SHORT = {"voxel_kernel": "vk", "voxel_walk": "walk", "voxel_overlap": "ov", "voxel_skip": "skip", "voxel_tight": "tight", "wide_drain": "wide",
         "coop_tail": "coop", "voxel_order": "ord", "ticket_rays": "tick", "k1p_static_rays": "stat", "batch_chunks": "chunks",
         "bounce_fused": "fused", "bounce_pack": "pack"}
ADJUST = {"excl": "hits", "tmax": "hits", "writeback": "outside", "bounce": "escape"}            # what a kind of reference needs from its rays (below: _rays)
N_DEGENERATE = 822                                               # what degenerate_rays yields (22 fixed rays, 400 + 400 drawn)


def _impossible():
    """{frozenset of two (factor, level)}: reason}"""
    t = {}
    for n in FACTORS["n"]:
        if n > N_DEGENERATE:
            t[frozenset({("rays", "degenerate"), ("n", n)})] = "degenerate_rays yields %d rays" % N_DEGENERATE
    for mode in FACTORS["mode"]:
        if mode != "bounce":
            t[frozenset({("mode", mode), ("bounce_fused", 1)})] = "bounce_fused is read by the bounce loop only: the case would be its twin with 0"
            t[frozenset({("mode", mode), ("bounce_pack", 0)})] = "bounce_pack is read by the bounce loop only: the case would be its twin with 1"
    t[frozenset({("mode", "own"), ("voxel_kernel", 1)})] = "K1p has no counting build: the call is refused (HARE_E_UNSUPPORTED)"
    t[frozenset({("mode", "bounce"), ("n", 1)})] = "one ray cannot both be alive at the third cast and have been retired before it"
    t[frozenset({("mode", "occl_tmax"), ("n", 1)})] = "one ray cannot hold five classes of t_max"
    t[frozenset({("bounce_fused", 1), ("n", 1)})] = "follows from the two above: only a bounce case sets it, and none has one ray"
    t[frozenset({("bounce_pack", 0), ("n", 1)})] = "follows from the two above: only a bounce case sets it, and none has one ray"
    return t


IMPOSSIBLE = _impossible()


class Case:
    """One setting of every factor.  kind: which reference the mode is compared with ("plain": the closest hit without exclusions)."""

    def __init__(self, index, **levels):
        if set(levels) != set(NAMES):
            raise ValueError("a case sets every factor: %s" % sorted(set(NAMES) ^ set(levels)))
        for k, v in levels.items():
            if v not in FACTORS[k]:
                raise ValueError("%s has no level %r" % (k, v))
        items = [(k, levels[k]) for k in NAMES]
        for a in range(len(items)):
            for b in range(a + 1, len(items)):
                why = IMPOSSIBLE.get(frozenset({items[a], items[b]}))
                if why:
                    raise ValueError("%s=%s with %s=%s: %s" % (items[a] + items[b] + (why,)))
        self.index, self.levels = index, dict(items)
        self.__dict__.update(levels)
        self.options = {k: levels[k] for k in OPTIONS}
        opts = "".join("-%s%d" % (SHORT[k], v) for k, v in self.options.items() if v != FACTORS[k][0])
        self.id = "%d-%s-%s-%s-n%d-%s%s" % (index, self.scene, self.grid, self.rays, self.n, self.mode, opts)
        self.kind = self.mode if self.mode in ("excl", "writeback", "retired", "bounce") else ("tmax" if self.mode == "occl_tmax" else "plain")
        assert self.n <= MAX_RAYS

    @property
    def adjust(self):
        return ADJUST.get(self.kind, "")

    @property
    def key(self):
        """what the inputs and the reference depend on"""
        return (self.scene, self.grid, self.rays, self.n, self.kind)

    @property
    def cell(self):
        """(family, coarse bitmap, quadrilaterals): the member of the voxel kernel table (device_scene.cpp: kVoxelKernelNames) that serves
        the case by launch.cpp's rule -- the fused bounce loop is one launch of `Bounce`, the loop of a launch per cast runs the others"""
        o = self.options
        if self.mode in ("occl", "occl_tmax"):
            fam = "Occl"
        elif self.mode == "own":
            fam = "PoolOwn"
        elif o["voxel_kernel"] == 1:
            fam = "Persist"
        elif self.mode == "bounce" and o["bounce_fused"] == 1:
            fam = "Bounce"
        else:
            fam = "PoolOv" if o["voxel_overlap"] == 1 else "Pool"
        return fam, int(self.grid in ("D81", "D161")), int(self.scene != "tie")


FAMILIES = ("Pool", "PoolOv", "PoolOwn", "Persist", "Occl", "Bounce")


# ------------------------------------------------------------------------------------------------------------ the covering array
def all_pairs():
    """every pair of levels of every two factors that is not declared impossible"""
    pairs = set()
    for a in range(len(NAMES)):
        for b in range(a + 1, len(NAMES)):
            for x in FACTORS[NAMES[a]]:
                for y in FACTORS[NAMES[b]]:
                    p = frozenset({(NAMES[a], x), (NAMES[b], y)})
                    if p not in IMPOSSIBLE:
                        pairs.add(p)
    return pairs


def pairs_of(levels):
    items = list(levels.items())
    return {frozenset({items[a], items[b]}) for a in range(len(items)) for b in range(a + 1, len(items))}


def _generate():
    """Greedy, one case at a time: start from an uncovered pair, give every other factor (in a drawn order) the level that covers the
    most pairs still uncovered with what is set, among the levels no declared pair forbids; the best of 24 such candidates is taken."""
    rng = np.random.default_rng(SEED)
    flat = [(k, v) for k in NAMES for v in FACTORS[k]]               # every level of every factor, numbered
    ids = {kv: i for i, kv in enumerate(flat)}
    of = {k: [ids[(k, v)] for v in FACTORS[k]] for k in NAMES}
    todo = np.zeros((len(flat), len(flat)), bool)                    # pairs still to cover / pairs declared impossible, both symmetric
    bad = np.zeros_like(todo)
    for p in all_pairs():
        i, j = (ids[kv] for kv in p)
        todo[i, j] = todo[j, i] = True
    for p in IMPOSSIBLE:
        i, j = (ids[kv] for kv in p)
        bad[i, j] = bad[j, i] = True
    out = []
    while todo.any():
        left = np.argwhere(np.triu(todo))
        best, best_gain = None, -1
        for trial in range(24):
            chosen = [int(i) for i in left[int(rng.integers(0, len(left))) if trial else 0]]
            for f in rng.permutation(len(NAMES)):
                k = NAMES[f]
                if any(flat[i][0] == k for i in chosen):
                    continue
                free = [i for i in of[k] if not bad[i, chosen].any()]
                if not free:
                    chosen = None
                    break
                score = [int(todo[i, chosen].sum()) for i in free]
                pick = [i for i, s in zip(free, score) if s == max(score)]
                chosen.append(pick[int(rng.integers(0, len(pick)))])
            if chosen is None:
                continue
            gain = int(todo[np.ix_(chosen, chosen)].sum()) // 2
            if gain > best_gain:
                best, best_gain = chosen, gain
        assert best is not None and best_gain > 0
        out.append(Case(len(out), **dict(flat[i] for i in best)))
        todo[np.ix_(best, best)] = False
    # a case in every cell of the kernel table the array left empty: first levels everywhere else, shapes and rays going round
    have = {c.cell for c in out}
    k = 0
    for fam in FAMILIES:
        for coarse in (0, 1):
            for quads in (0, 1):
                if (fam, coarse, quads) in have:
                    continue
                lv = {name: FACTORS[name][0] for name in NAMES}
                lv["scene"] = ("soup", "two")[k % 2] if quads else "tie"
                lv["grid"] = (("D81", "D161") if coarse else ("D33", "A7", "D8"))[k % (2 if coarse else 3)]
                lv["rays"] = ("face", "awkward", "soup", "tie")[k % 4]
                lv["n"] = FACTORS["n"][3 + k % 4]
                lv["mode"] = {"Occl": "occl_tmax", "PoolOwn": "own", "Bounce": "bounce"}.get(fam, ("excl", "closest", "writeback")[k % 3])
                lv["voxel_kernel"] = 1 if fam == "Persist" else 2
                lv["voxel_overlap"] = 1 if fam == "PoolOv" else 0
                lv["bounce_fused"] = 1 if fam == "Bounce" else 0
                out.append(Case(len(out), **lv))
                assert out[-1].cell == (fam, coarse, quads)
                k += 1
    return out


# --------------------------------------------------------------------------------------------------------------- scenes and grids
@lru_cache(maxsize=None)
def scene_of(name):
    """(polygons of every topology [(verts, nverts), ...], the topology that is shot, size), read-only"""
    if name == "tie":
        v, nv, size = tie_scene()
        tops, top = [(v, nv)], 0
    elif name == "soup":
        v, nv, size = soup(n_tri=700, n_quad=300, seed=21)
        tops, top = [(v, nv)], 0
    else:                                   # a grid over two topologies, shot at the second (its lists are the second's, its boxes too)
        v0, n0, size = soup()
        v1, n1, _ = soup(n_tri=300, n_quad=80, seed=9, size=(5.0, 4.5, 3.5))
        tops, top = [(v0, n0), (v1, n1)], 1
    for v, nv in tops:
        v.flags.writeable = False
        nv.flags.writeable = False
    return tops, top, tuple(size)


def scene(case):
    return scene_of(case.scene)


def grid_args(grid):
    """(Domain, Avg_polys or None) of Voxel_Grid's constructors"""
    return (7, 12) if grid == "A7" else (int(grid[1:]), None)


@lru_cache(maxsize=None)
def oracle_topologies(scene_name):
    return [po.Topology(v, nv) for v, nv in scene_of(scene_name)[0]]


class _Shot:
    """an oracle grid shot at one topology, with the .shoot oracle_bounce_loop calls"""

    def __init__(self, grid, top):
        self.grid, self.top = grid, top

    def shoot(self, rays, **kw):
        return self.grid.shoot(rays, top_index=self.top, **kw)


@lru_cache(maxsize=None)
def oracle_grid(scene_name, grid):
    D, avg = grid_args(grid)
    T = oracle_topologies(scene_name)
    g = po.VoxelGrid(T, domain=D) if avg is None else po.VoxelGrid(T, max_domain=D, avg_polys=avg)
    return _Shot(g, scene_of(scene_name)[1])


# ----------------------------------------------------------------------------------------------------------------------- inputs
def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _generated(scene_name, grid, rays, n):
    tops, top, size = scene_of(scene_name)
    v, nv = tops[top]
    D = grid_args(grid)[0]
    seed = _seed(scene_name, rays, n) % 1000
    if rays == "tie":
        return tie_rays(v, nv, size, n=n, seed=seed)
    if rays == "face":
        return face_rays(v, nv, size, n=n, seed=seed)
    if rays == "awkward":
        return awkward_rays(size, vd_hint=(size[0] + 0.202) / D, n=n, seed=seed)
    if rays == "soup":
        return soup_rays(n, size, seed=seed)
    r = degenerate_rays(size, D, seed=seed)
    assert len(r) == N_DEGENERATE
    return np.ascontiguousarray(r[np.random.default_rng(seed).permutation(len(r))[:n]])


@lru_cache(maxsize=None)
def _rays(scene_name, grid, rays, n, adjust):
    size = np.asarray(scene_of(scene_name)[2])
    if n == 1:                              # the generator's first ray the plain cast hits (the first ray where none does)
        r = _generated(scene_name, grid, rays, WAVE)
        hit = np.nonzero(oracle_grid(scene_name, grid).shoot(r)[0]["hit"])[0]
        r = np.ascontiguousarray(r[hit[0]:hit[0] + 1] if hit.size else r[:1])
    else:
        r = _generated(scene_name, grid, rays, n)
    assert r.shape == (n, 6)
    k = np.arange(n)
    if adjust == "hits" and n > 1:          # two rays of five turned towards a point inside a drawn polygon, from where they start
        tops, top, _ = scene_of(scene_name)
        v = tops[top][0]
        rng = np.random.default_rng(_seed(scene_name, grid, rays, n, "aim"))
        p = rng.integers(0, len(v), n)
        aim = v[p, 0] + 0.3 * (v[p, 1] - v[p, 0]) + 0.3 * (v[p, 2] - v[p, 0])
        sel = np.isin(k % 5, (0, 2)) & np.isfinite(r[:, :3]).all(axis=1)
        r[sel, 3:] = (aim - r[:, :3])[sel]
    elif adjust == "outside":                 # against the direction, two diagonals back: the origin is outside, the grid ahead
        d = r[:, 3:]
        with np.errstate(all="ignore"):
            u = d / np.linalg.norm(d, axis=1, keepdims=True)
        sel = (k % 4 == 0) & np.isfinite(u).all(axis=1) & np.isfinite(r[:, :3]).all(axis=1)
        r[sel, :3] -= u[sel] * 2.0 * np.linalg.norm(size)
    elif adjust == "escape":                # behind the far corner, flying away
        sel = k % 4 == 2
        r[sel, :3] = size * 1.5 + 1.0
        r[sel, 3:] = (1.0, 0.5, 0.25)
    r.flags.writeable = False
    return r


def rays(case):
    """float64 [n, 6], read-only"""
    return _rays(case.scene, case.grid, case.rays, case.n, case.adjust)


def tmax_of(ref, seed):
    """t_max as tests/test_gpu_round5.py makes it for the kd-tree's occlusion kernel: a multiple of every ray's own hit distance, a drawn
    value for a ray without a hit, EXACTLY the hit distance and one ulp beyond it on every seventh of the rays that hit, and inf / NaN / -1 / 0 on
    four rays of every eleven"""
    rng = np.random.default_rng(seed)
    n = len(ref)
    t = ref["t"].copy()
    hit = ref["hit"] != 0
    tmax = t * rng.choice([0.3, 0.999999, 1.0, 1.000001, 3.0], n)
    tmax[~hit] = rng.uniform(0.1, 30.0, int((~hit).sum()))
    k = np.cumsum(hit) - 1                  # a ray's number among those that hit
    a, b = hit & (k % 7 == 1), hit & (k % 7 == 2)
    tmax[a] = t[a]
    tmax[b] = np.nextafter(t[b], np.inf)
    tmax[3::11] = np.inf; tmax[4::11] = np.nan; tmax[5::11] = -1.0; tmax[6::11] = 0.0
    return tmax


@lru_cache(maxsize=None)
def _plain(scene_name, grid, rays, n, adjust):
    ev, c = oracle_grid(scene_name, grid).shoot(_rays(scene_name, grid, rays, n, adjust))
    ev.flags.writeable = False
    return ev, c


@lru_cache(maxsize=None)
def _reference(key):
    scene_name, grid, rays_name, n, kind = key
    adjust = ADJUST.get(kind, "")
    o = oracle_grid(scene_name, grid)
    tops, top, _ = scene_of(scene_name)
    P = len(tops[top][1])
    r = _rays(scene_name, grid, rays_name, n, adjust)
    plain, pc = _plain(scene_name, grid, rays_name, n, adjust)
    rng = np.random.default_rng(_seed(key))
    ref = {"plain": plain, "e1": None, "e2": None}
    if kind == "plain":
        ev, c = plain, pc
        ref["occ_any"] = (plain["hit"] != 0).astype(np.int32)
    elif kind == "tmax":
        ev, c = plain, pc
        ref["tmax"] = tmax_of(plain, _seed(key, "tmax"))
        with np.errstate(invalid="ignore"):
            ref["occ_tmax"] = ((plain["hit"] != 0) & (plain["t"] < ref["tmax"])).astype(np.int32)
    elif kind == "excl":                    # leave the polygon the plain cast hits; a drawn second exclusion; indices that match no polygon
        hit = plain["hit"] != 0
        ref["e1"] = np.where(hit, plain["poly_id"], rng.integers(-3, P, n)).astype(np.int32)
        ref["e2"] = rng.integers(-3, P, n).astype(np.int32)
        ref["e2"][1::5] = -1 - np.arange(len(ref["e2"][1::5])) % 3
        ev, c = o.shoot(r, excl1=ref["e1"], excl2=ref["e2"])
    elif kind == "writeback":
        ev, c, ref["moved"] = o.shoot(r, mutate=True)
    elif kind == "retired":                 # every third ray is retired (-2): its record is X_Event() and it is not counted
        e1 = np.where(rng.random(n) < 0.5, plain["poly_id"], rng.integers(-1, P, n)).astype(np.int32)
        e1[::3] = -2
        live = e1 != -2
        ev = np.zeros(n, po.XEVENT_DTYPE)
        ev["poly_id"] = -1
        c = {"rays": 0, "hits": 0}
        if live.any():
            ev[live], c = o.shoot(r[live], excl1=e1[live])
        ref["e1"] = e1
    else:                                   # the bounce loop, cast by cast
        ev, per_cast = oracle_bounce_loop(po, oracle_topologies(scene_name)[top], o, r, BOUNCES, nthreads=4)
        ref["per_cast"] = per_cast
        c = {"rays": sum(p["rays"] for p in per_cast), "hits": sum(p["hits"] for p in per_cast)}
    ref["events"], ref["rays"], ref["hits"] = ev, int(c["rays"]), int(c["hits"])
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return ref


def reference(case):
    """The oracle's answer, shared by every case of the same key: dict of `events` ([n], or [3, n] for the bounce loop), `rays` and `hits`
    (the counters), `plain` (the closest hit without exclusions on the same rays), `e1` / `e2` (the exclusions of the call, or None), and by
    kind `moved` (write-back: the rays as the reference leaves them), `occ_any` (plain: the flags of an occlusion call without t_max), `tmax`
    / `occ_tmax` (tmax: the input and the flags of one with), `per_cast` (bounce: the counters of every cast)."""
    return _reference(case.key)


CASES = _generate()
