"""Inputs for the receive loop's device tests (include/hare_hip.h, "receivers"): case records built from numpy and the oracle alone, no
GPU.  Case is the one record of every set -- the two below, the termination rules' (tests/receive_cut_ref.py) and the receiver maps'
(tests/receive_map_ref.py) -- and reference(case) the one way from a case to what the library must return.  Two sets here.  edge_cases(): fixed, hand-built states and parameters at the numeric edges of the definition -- "0 unless > 0",
min(., 2^63), rint's ties, the NaN branch and the +-2^62 clamp of the directional words, sums that wrap, x exactly on a bin edge and
exactly at n_bins, detections that are not binned -- at every band count, at K up to 256, at batch sizes around a wave, a workgroup and
the live-block list's threshold, with poly_origin1 / poly_origin2 on the first cast.  sweep_case(seed): one case drawn from a seed over the
whole parameter space (tools/fuzz_receive.py runs them by the thousand).  reference(case) runs tests.receive_ref.receive_loop on a case and
returns what the library must return, byte for byte, with the tallies that say which edge classes the case went through
(tests/test_receive_cases.py asserts that the sets hold what they claim to hold).  digest(result) is the SHA-256 that
tests/golden/receive_reference_digests.json pins for every fixed case and sweep seed (tests/test_receive_reference_pinned.py)."""
import dataclasses
import functools
import hashlib
import json
import os

import numpy as np

import hare_amd.scenes as scenes
from oracle import pyoracle as po
from tests.helpers import soup, soup_rays
from tests.receive_ref import receive_loop

MODES = ("specular", "scatter", "rain")
TWO63, TWO62 = 2.0 ** 63, 2.0 ** 62
WORDS_MAX = 1 << 27                      # K x n_bins x B (x 4) of a receive call
TINY = 2.0 ** -600                       # a direction scaled by it: dx*dx underflows to 0, every other product stays a normal number

# the state planes of the edge cases are drawn from these
E_SPECIAL = (np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 0.5, 1.5, 2.5, 5e-324, 1e300, TWO63, TWO62, 2.0 ** -62, 1.0)
L_SPECIAL = (0.0, -0.0, -1.0, -0.5, np.nan, np.inf, -np.inf, 1e300)


@dataclasses.dataclass
class Case:
    name: str
    scene: tuple                         # ("shoebox",) | ("room",) | ("soup", n_tri, n_quad, seed) | ("box", sx, sy, sz, tx, ty, tz)
    partition: tuple                     # ("voxel", domain) | ("octree", depth, max_polys) | ("kdtree", depth, max_polys)
    rays: np.ndarray                     # [n, 6]
    bounces: int
    centers: np.ndarray                  # [K, 3]
    radii: np.ndarray                    # [K]
    n_bins: int
    bin_len: float
    frac_bits: int
    mode: str = "specular"               # MODES
    directional: bool = False
    aggregate: int = 1                   # scene option "receive_aggregate"
    pack: int = 1                        # scene option "bounce_pack"
    alpha: np.ndarray = None             # [P, B] or None
    sigma: np.ndarray = None             # [P, B]; None in specular mode
    state_in: np.ndarray = None          # [1 + B, n] or None (L = 0, E = 1)
    seed: int = 0                        # scene option "scatter_seed"
    excl1: np.ndarray = None             # poly_origin1 / poly_origin2 of the first cast
    excl2: np.ndarray = None
    shards: int = 1                      # 2: Receive_batch_sharded over two partitions
    device: bool = False                 # also through receive_device with caller-owned buffers
    time_limit: bool = False             # HARE_RECEIVE_TIME_LIMIT
    floor_bits: int = 0                  # scene option "receive_floor_bits"
    roulette: bool = False               # scene option "receive_roulette"
    map_cell: float = None               # None: the linear receiver loop; >= 0: a receiver map with this `cell` (0: the default)
    map_shape: str = None                # tests.receive_map_ref.map_layout's shape (for describe() only)
    two_scenes: bool = False             # also through Receive_batch_sharded over two scenes

    @property
    def n(self):
        return self.rays.shape[0]

    @property
    def K(self):
        return self.centers.shape[0]

    @property
    def B(self):
        for t in (self.alpha, self.sigma):
            if t is not None:
                return t.shape[1]
        return 1

    @property
    def words(self):
        return self.K * self.n_bins * self.B * (4 if self.directional else 1)

    def describe(self):
        rules = f" time_limit={int(self.time_limit)} floor_bits={self.floor_bits} roulette={int(self.roulette)}"
        return (f"{self.name}: {' '.join(str(x) for x in self.scene)} {' '.join(str(x) for x in self.partition)} n={self.n} bounces={self.bounces} "
                f"K={self.K} B={self.B} {self.mode}{' directional' if self.directional else ''} aggregate={self.aggregate} pack={self.pack} "
                f"frac_bits={self.frac_bits} n_bins={self.n_bins} bin_len={self.bin_len!r} state_in={self.state_in is not None} "
                f"seed={self.seed} excl={self.excl1 is not None} shards={self.shards}"
                f"{rules if self.time_limit or self.floor_bits or self.roulette else ''}"
                f"{'' if self.map_cell is None else f' map={self.map_shape} cell={self.map_cell!r}'}")

    def without(self, **fields):
        """The case with some fields replaced (the rules switched off, say); it keeps its name."""
        return dataclasses.replace(self, **fields)


def partition_room():
    """tests.test_gpu_rain.partition_room (that module needs a GPU to import): the shoebox with an interior wall at x = 5, y = 0 .. 4.2."""
    m = scenes.shoebox()
    wall = scenes._patch([5.0, 0.0, 0.0], [0.0, 4.2, 0.0], [0.0, 0.0, 4.0], 3, 3)
    v = np.zeros((wall.shape[0], 4, 3))
    v[:, :3] = wall
    return np.concatenate([m.verts, v]), np.concatenate([m.nverts, np.full(wall.shape[0], 3, np.int32)]), m.size


_MESHES = {}


def mesh_of(scene):
    """(verts [P, 4, 3], nverts [P], size) of a case's scene."""
    if scene not in _MESHES:
        if scene[0] == "shoebox":
            m = scenes.shoebox()
            _MESHES[scene] = (m.verts, m.nverts, m.size)
        elif scene[0] == "room":
            _MESHES[scene] = partition_room()
        elif scene[0] == "box":          # the shoebox mapped by a per-axis scale and a shift: x' = x * s + t; size is the scaled one
            m = scenes.shoebox()
            s, t = np.array(scene[1:4], np.float64), np.array(scene[4:7], np.float64)
            used = np.arange(4)[None, :, None] < m.nverts[:, None, None]
            _MESHES[scene] = (np.ascontiguousarray(np.where(used, m.verts * s + t, 0.0)), m.nverts, tuple(np.asarray(m.size) * s))
        else:
            _MESHES[scene] = soup(n_tri=scene[1], n_quad=scene[2], seed=scene[3])
    return _MESHES[scene]


_ORACLES = {}


def oracle_of(case):
    """(oracle topology, oracle partition) of a case; kept, as the cases share a handful of them."""
    key = (case.scene, case.partition)
    if key not in _ORACLES:
        verts, nverts, _ = mesh_of(case.scene)
        To = po.Topology(verts, nverts)
        kind, *par = case.partition
        o = po.VoxelGrid([To], domain=par[0]) if kind == "voxel" else (po.Octree if kind == "octree" else po.KDTree)([To], *par)
        if len(_ORACLES) > 8:
            _ORACLES.clear()
        _ORACLES[key] = (To, o)
    return _ORACLES[key]


_REFERENCES = {}
REFERENCES_KEPT = 160                    # the fixed sets and their rules-off variants together are about a hundred


def reference(case, counts=False, nthreads=16, keep=False, candidates_fn=None):
    """tests.receive_ref.receive_loop on the case: dict with hist, det, state and rays as that function returns them, events (the last
    cast's), stats (the rain's eligible / occluded queries), tallies (receive_ref.TALLIES), counts [K, n_bins] (on request, else None),
    per_cast (live rays, the rules' retirements and the roulette's survivors per cast) and share ((candidate pairs, pairs) per receiver
    step of a map; empty without one) and map_tallies (tests.receive_map_ref.MAP_TALLIES, the classes of the visit rule the casts went
    through, summed over the casts; empty without a map).  candidates_fn: a visit rule to run in place of
    tests.receive_map_ref.candidates (a test's variant of the rule; never kept).  keep: the result is kept, and served from then on, under the case's name and what separates
    two cases of one name (`without` variants) -- for the fixed sets, whose tests share it and leave it unchanged; the oldest of more
    than REFERENCES_KEPT goes."""
    key = (case.name, case.time_limit, case.floor_bits, case.roulette, case.map_cell, counts)
    assert candidates_fn is None or not keep
    if key in _REFERENCES and candidates_fn is None:
        return _REFERENCES[key]
    To, o = oracle_of(case)
    stats, tallies, last, per_cast, share, map_tallies = {}, {}, [], {}, [], {}
    cnt = np.zeros((case.K, case.n_bins), np.int64) if counts else None
    visit = None
    if case.map_cell is not None:
        from tests.receive_map_ref import build_grid, candidates          # that module builds its cases from this one's
        visit = functools.partial(candidates_fn or candidates, build_grid(case.centers, case.radii, case.map_cell), tallies=map_tallies, centers=case.centers,
                                  radii=case.radii)
    hist, det, state, rays = receive_loop(po, To, o, case.rays, case.bounces, case.centers, case.radii, case.n_bins, case.bin_len, case.frac_bits,
                                          alpha=case.alpha, sigma=case.sigma if case.mode != "specular" else None, seed=case.seed,
                                          state_in=case.state_in, rain=case.mode == "rain", directional=case.directional, stats=stats,
                                          counts=cnt, nthreads=nthreads, tallies=tallies, excl1=case.excl1, excl2=case.excl2, last_events=last,
                                          time_limit=case.time_limit, floor_bits=case.floor_bits, roulette=case.roulette, visit=visit,
                                          per_cast=per_cast, share=share)
    out = dict(hist=hist, det=det, state=state, rays=rays, events=last[0], stats=stats, tallies=tallies, counts=cnt, per_cast=per_cast,
               share=share, map_tallies=map_tallies)
    if keep:
        if len(_REFERENCES) >= REFERENCES_KEPT:
            del _REFERENCES[next(iter(_REFERENCES))]
        _REFERENCES[key] = out
    return out


def digest(out, per_cast=False):
    """SHA-256 (hex) over a reference result: hist, det, state, rays, every field of the last events and, on request, per_cast's four
    arrays; of each its name, dtype, shape and bytes, every NaN first replaced by one bit pattern (its sign and payload are the FPU's,
    DESIGN.md 1)."""
    h = hashlib.sha256()
    arrays = [(k, out[k]) for k in ("hist", "det", "state", "rays")] + [("events." + f, out["events"][f]) for f in out["events"].dtype.names]
    if per_cast:
        arrays += [("per_cast." + k, out["per_cast"][k]) for k in ("live", "time", "floor", "boosted")]
    for name, a in arrays:
        a = np.ascontiguousarray(a)
        if a.dtype.kind == "f":
            assert a.dtype == np.float64, (name, a.dtype)
            a = a.copy()
            a.view(np.uint64)[np.isnan(a)] = np.uint64(0x7FF8000000000000)
        h.update(f"{name} {a.dtype.str} {a.shape}\n".encode())
        h.update(a.tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def pinned_digests():
    """tests/golden/receive_reference_digests.json: digest() of every fixed case ("edge/", "cut/", "map/", "identity/" + name), of the
    sweeps' seeds ("sweep/" 0 .. 199, "sweep-cut/" 0 .. 39) and of four rules' cases with the rules off ("rules-off/"), as the three
    loops that receive_loop replaced returned them; per_cast is in the digest of "cut/" and "sweep-cut/"."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "receive_reference_digests.json")) as f:
        return json.load(f)


def wave_counts(case, w):
    """The adds per (receiver, bin) [K, n_bins] of the first cast of rays 64 w .. 64 w + 63: the lanes of one wave."""
    s = slice(64 * w, min(64 * w + 64, case.n))
    sub = dataclasses.replace(case, rays=case.rays[s], bounces=1, state_in=None if case.state_in is None else case.state_in[:, s],
                              excl1=None if case.excl1 is None else case.excl1[s], excl2=None if case.excl2 is None else case.excl2[s])
    return reference(sub, counts=True)["counts"]


# ---- tables
def alpha_table(P, B, rng):
    a = rng.uniform(0.0, 0.6, (P, B))
    a[::17] = 0.0
    a[5::23] = 1.0                       # full absorption: E becomes 0 (or NaN from inf), the ray lives on
    return a


def sigma_table(P, B, rng):
    s = rng.uniform(0.0, 1.0, (P, B))
    s[::13] = 0.0                        # specular polygons
    s[4::19] = 1.0                       # fully diffuse ones
    if B > 1:
        s[7::11, 0] = 0.0
        s[7::11, B - 1] = 1.0
    return s


# ---- edge cases
def edge_L(k, bin_len):
    """A double L with L / bin_len == k exactly (x on the lower edge of bin k; k = n_bins: the first value that is not binned)."""
    v = np.float64(k) * np.float64(bin_len)
    for c in (v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)):
        if c / np.float64(bin_len) == np.float64(k):
            return float(c)
    raise AssertionError((k, bin_len))


def edge_state(n, B, n_bins, bin_len, rng, spread):
    """[1 + B, n]: two rays in three take L and every E from the special values (every pairing comes up: the strides are coprime to the
    lists' lengths), the others ordinary ones.  spread: the ordinary L of ray i is bin (37 i mod n_bins)'s lower edge plus a quarter
    bin, so that the lanes of a wave fall into distinct bins; otherwise it is drawn over 1.1 times the histogram's length."""
    Ls = list(L_SPECIAL) + [0.3 * bin_len, 1.7 * bin_len] + [edge_L(k, bin_len) for k in sorted({0, 1, n_bins // 2, n_bins - 1, n_bins})]
    i = np.arange(n)
    if spread:
        L = np.array([edge_L(int(k), bin_len) for k in (37 * i) % n_bins]) + 0.25 * bin_len
    else:
        L = rng.uniform(0.0, 1.1 * n_bins * bin_len, n)
    special = i % 3 != 2
    if not spread:
        L[special] = np.array(Ls)[(i[special] * 5 + 1) % len(Ls)]
    st = np.empty((1 + B, n))
    st[0] = L
    for b in range(B):
        E = rng.uniform(0.0, 2.0, n)
        E[special] = np.array(E_SPECIAL)[(i[special] * 7 + 4 * b) % len(E_SPECIAL)]
        st[1 + b] = E
    return st


def edge_receivers(size, K, rng):
    """K receivers of which the first three in four are centred on the burst's source, coincident and nested (radii from five values):
    every ray of the burst passes every one of them at s = 0, so x = L / bin_len exactly.  The others lie about the room."""
    S = np.array([0.31, 0.42, 0.37]) * np.asarray(size)                  # hare_amd.scenes.burst_rays
    at = max(1, (3 * K) // 4)
    c = np.concatenate([np.broadcast_to(S, (at, 3)), rng.uniform(0.15, 0.85, (K - at, 3)) * np.asarray(size)])
    r = np.concatenate([np.array([0.25, 0.5, 0.5, 1.0, 0.125])[np.arange(at) % 5], rng.uniform(0.3, 0.9, K - at)])
    return np.ascontiguousarray(c), r


def edge_case(name, scene="shoebox", partition=("voxel", 8), n=4159, K=3, B=1, mode="specular", directional=False, aggregate=1, frac_bits=0,
              bounces=2, n_bins=64, bin_len=0.0625, spread=False, excl=False, tiny=False, device=False, pack=1, seed=5):
    rng = np.random.default_rng(1000 * n + 10 * K + B)
    verts, nverts, size = mesh_of((scene,))
    P = verts.shape[0]
    if mode == "rain":
        bounces = 2                       # the rain falls between two casts
    rays = scenes.burst_rays(n, size)
    if tiny:
        rays[17::64, 3:] *= TINY          # len = 0: a lane that detects nothing and whose arrival vector is -(d / 0)
    centers, radii = edge_receivers(size, K, rng)
    alpha = alpha_table(P, B, rng) if B > 1 or (mode == "specular" and K % 2 == 0) else None
    sigma = sigma_table(P, B, rng) if mode != "specular" else None
    e1 = e2 = None
    if excl:
        e1 = rng.integers(-1, P, n).astype(np.int32)
        e2 = rng.integers(-1, P, n).astype(np.int32)
    return Case(name, (scene,), partition, rays, bounces, centers, radii, n_bins, bin_len, frac_bits, mode, directional, aggregate, pack, alpha, sigma,
                edge_state(n, B, n_bins, bin_len, rng, spread), seed, e1, e2, 1, device)


def edge_cases():
    """The fixed set.  Every case takes its state from edge_state; between them they cover the six kernel forms with the aggregated and
    the per-lane add, frac_bits 0 / 1 / 62, B = 1 .. 8, K = 1 / 64 / 255 / 256, the batch sizes about a wave, a workgroup and 4096,
    bounces 1 and 2, n_bins = 1 and a wide histogram with a wave's lanes in distinct bins, and exclusions on the first cast."""
    out = []
    fracs = (0, 1, 62)
    # the six forms x aggregate, in the partition room (its wall occludes some of the rain's queries), B and frac_bits rotating
    j = 0
    for mode in MODES:
        for directional in (False, True):
            for agg in (1, 0):
                out.append(edge_case(f"form-{mode}-{int(directional)}-{agg}", scene="room", n=4159, K=3, B=(5, 8, 3)[j % 3], mode=mode,
                                     directional=directional, aggregate=agg, frac_bits=fracs[j % 3], device=agg == 1 and mode != "scatter"))
                j += 1
    # every band count, aggregated: the lane maps lane == b and (lane & 15) == b.  A fresh scene each, as B is fixed per scene
    for B in range(1, 9):
        for directional in (False, True):
            out.append(edge_case(f"bands-{B}-{int(directional)}", n=257, K=4, B=B, mode=MODES[B % 3], directional=directional,
                                 frac_bits=fracs[B % 3], bounces=1 + B % 2))
    # the batch sizes: workgroups and waves partly past n, the live-block list's threshold
    for j, n in enumerate((1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)):
        out.append(edge_case(f"n-{n}", n=n, K=2, B=(1, 2, 4, 7)[j % 4], mode=MODES[j % 3], directional=j % 2 == 1, frac_bits=fracs[j % 3],
                             bounces=1 + j % 2, device=n in (1, 65, 4095, 4096), pack=1 if n != 4097 else 0))
    # the receiver counts: the LDS staging loop (256 threads x 4 doubles per pass) up to its last slot
    for j, K in enumerate((1, 64, 255, 256)):
        out.append(edge_case(f"K-{K}", n=320, K=K, B=(6, 2, 1, 3)[j], mode=MODES[j % 3], directional=j % 2 == 0, frac_bits=fracs[j % 3],
                             n_bins=16))
    # one bin; and a wide histogram whose bins are short: the longest form of the rounds over a wave's distinct bins
    for directional in (False, True):
        out.append(edge_case(f"one-bin-{int(directional)}", n=4097, K=3, B=2, directional=directional, frac_bits=62, n_bins=1, bin_len=0.5))
        out.append(edge_case(f"distinct-bins-{int(directional)}", n=4159, K=2, B=3, directional=directional, frac_bits=1, n_bins=4096,
                             bin_len=2.0 ** -9, spread=True, bounces=1 + int(directional), device=True))
    out.append(edge_case("bin-len-0.05", n=4159, K=3, B=4, mode="rain", directional=True, frac_bits=1, n_bins=600, bin_len=0.05))
    # poly_origin1 / poly_origin2 on the first cast
    for j, mode in enumerate(MODES):
        out.append(edge_case(f"excl-{mode}", scene="room", n=4097, K=3, B=2 + j, mode=mode, directional=j != 1, frac_bits=fracs[j], excl=True,
                             device=j != 1, partition=(("voxel", 8), ("octree", 4, 8), ("kdtree", 8, 6))[j]))
    # lanes whose arrival vector is not a number beside lanes that deposit (specular only: a diffuse direction is w * len = 0)
    for agg in (1, 0):
        out.append(edge_case(f"tiny-{agg}", n=4159, K=3, B=5, directional=True, aggregate=agg, frac_bits=62, tiny=True, device=agg == 1))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


# ---- sweep cases
def sweep_case(seed):
    """One case from the seed.  Nothing is redrawn: every draw is accepted as it comes, and receiver 0 lies on ray 0's path."""
    rng = np.random.default_rng(0x5EED0000 + int(seed))
    which = int(rng.integers(0, 4))
    if which <= 1:
        scene = ("soup", int(rng.integers(20, 500)), int(rng.integers(0, 150)), int(rng.integers(0, 1000)))
    else:
        scene = ("shoebox",) if which == 2 else ("room",)
    verts, nverts, size = mesh_of(scene)
    P = verts.shape[0]
    kind = ("voxel", "octree", "kdtree")[int(rng.integers(0, 3))]
    if kind == "voxel":
        partition = ("voxel", int(rng.choice([1, 2, 5, 8, 13, 31])))
    elif kind == "octree":
        partition = ("octree", int(rng.integers(0, 3)), int(rng.integers(1, 40)))     # nodes stay above 1 m (the reference's 0.1 m padding)
    else:
        partition = ("kdtree", int(rng.integers(0, 11)), int(rng.integers(1, 40)))
    # n: 1 .. about 20 000, half of them a multiple of 64 +- 1 or about the live-block list's threshold
    r = rng.random()
    if r < 0.3:
        n = max(1, 64 * int(rng.integers(1, 300)) + int(rng.integers(-1, 2)))
    elif r < 0.5:
        n = 4096 + int(rng.integers(-2, 3))
    else:
        n = int(np.exp(rng.uniform(0.0, np.log(20000.0))))
    if scene[0] == "soup" and rng.random() < 0.7:
        rays = soup_rays(n, size, seed=int(rng.integers(0, 1 << 30)))
    elif rng.random() < 0.5:
        rays = scenes.burst_rays(n, size)
    else:
        rays = scenes.random_rays(n, size, seed=int(rng.integers(1, 1 << 30)))
    bounces = int(rng.integers(1, 9))
    K = min(256, int(np.exp(rng.uniform(0.0, np.log(257.0)))))
    B = int(rng.integers(1, 9))
    mode = MODES[int(rng.integers(0, 3))]
    directional = bool(rng.integers(0, 2))
    centers = rng.uniform(-0.3, 1.3, (K, 3)) * np.asarray(size)                       # some outside the model
    radii = rng.uniform(0.1, 1.2, K)
    # receiver 0 on ray 0's path: half way to its first hit, or a unit along a ray that leaves
    To = po.Topology(verts, nverts)
    ev = po.brute(To, rays[:1])
    ev = ev[0] if isinstance(ev, tuple) else ev
    t = float(ev["t"][0]) * 0.5 if int(ev["hit"][0]) == 1 else 1.0
    centers[0] = rays[0, :3] + rays[0, 3:] * t
    alpha = sigma = None
    if B > 1 or rng.random() < 0.5:
        alpha = rng.uniform(0.0, 0.7, (P, B))
        alpha[rng.random(P) < 0.1] = 0.0
        alpha[rng.random(P) < 0.05] = 1.0
    if mode != "specular":
        sigma = rng.uniform(0.0, 1.0, (P, B))
        sigma[rng.random(P) < 0.15] = 0.0
        sigma[rng.random(P) < 0.15] = 1.0
    frac_bits = int(rng.integers(0, 63))
    n_bins = int(np.exp(rng.uniform(0.0, np.log(2001.0))))
    bin_len = float(np.exp(rng.uniform(np.log(1e-3), np.log(10.0))))
    state_in = None
    if rng.random() < 0.5:
        state_in = np.concatenate([rng.uniform(-0.5 * bin_len, 1.05 * n_bins * bin_len, (1, n)), rng.uniform(0.0, 2.0, (B, n))])
        if rng.random() < 0.4:                                                        # a sprinkle of the special values
            for row in range(1 + B):
                at = rng.random(n) < 0.1
                state_in[row, at] = rng.choice(np.array(E_SPECIAL if row else L_SPECIAL), int(at.sum()))
    scatter_seed = int(rng.integers(-(1 << 63), (1 << 63) - 1, endpoint=True))
    shards = 2 if rng.random() < 0.25 else 1
    case = Case(f"sweep-{seed}", scene, partition, np.ascontiguousarray(rays), bounces, centers, radii, n_bins, bin_len, frac_bits, mode, directional,
                int(rng.integers(0, 2)), int(rng.integers(0, 2)), alpha, sigma, state_in, scatter_seed, None, None, shards, False)
    assert case.words <= WORDS_MAX
    return case
