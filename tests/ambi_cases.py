"""The cases of the higher-order receivers' tests (include/hare_hip.h, "receivers", "Higher orders"): tests.receive_cases.Case with an
ambisonic order beside `directional`, built as that module builds its cases, and their reference -- tests.ambi_ref around
tests.receive_cases.reference.  tests/golden/ambi_reference_digests.json pins what the reference returns for every fixed case and for the
sweep's seeds (tests/test_ambi_reference.py); the GPU tests (tests/test_gpu_ambi*.py) compare the library with it byte for byte."""
import dataclasses
import functools
import json
import os

import numpy as np

import hare_amd.scenes as scenes
from tests import ambi_ref
from tests import receive_cases as rc

SHOEBOX12 = ("shoebox12",)               # the 12-triangle shoebox: one quad pair per face
SIZES = (63, 4097, 4159)                 # under a wave; a workgroup edge + 1 and + 63
BANDS = (1, 3, 8)                        # B = 8: 72 and 128 words per bin, more than a wave has lanes


def _register():
    """The 12-triangle shoebox under a scene name of its own in receive_cases' mesh table."""
    if SHOEBOX12 not in rc._MESHES:
        m = scenes.shoebox(nface=1)
        rc._MESHES[SHOEBOX12] = (m.verts, m.nverts, m.size)
    return rc._MESHES[SHOEBOX12]


@dataclasses.dataclass
class AmbiCase(rc.Case):
    order: int = 3                       # 2: HARE_RECEIVE_ORDER2 (nine channels), 3: HARE_RECEIVE_ORDER3 (sixteen)

    @property
    def channels(self):
        return ambi_ref.CHANNELS[self.order] if self.directional else 1

    @property
    def words(self):
        return self.K * self.n_bins * self.B * self.channels

    def describe(self):
        return super().describe() + f" order={self.order}"


def with_order(case, order, **fields):
    """A receive_cases.Case (directional) as an AmbiCase of this order."""
    kw = {f.name: getattr(case, f.name) for f in dataclasses.fields(rc.Case)}
    kw.update(fields)
    return AmbiCase(order=order, directional=True, **{k: v for k, v in kw.items() if k != "directional"})


_REFS = {}


def reference(case, nthreads=16):
    """tests.receive_cases.reference on the case with the deposit of its order: the same dict, hist [K, n_bins, B, C].  Kept per case
    name and order; the tests leave it unchanged."""
    key = (case.name, case.order, case.map_cell)
    if key not in _REFS:
        if len(_REFS) > 64:
            _REFS.clear()
        _REFS[key] = ambi_ref.run(case.order, rc.reference, case, nthreads=nthreads)
    return _REFS[key]


def digest(out):
    return rc.digest(out)


@functools.lru_cache(maxsize=None)
def pinned_digests():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ambi_reference_digests.json")) as f:
        return json.load(f)


# ---- the shoebox burst
def burst_receivers(size):
    """K = 3: a receiver of 1 m radius 2 m from the burst's source along its ray 0 (the pole of the burst: consecutive rays, the lanes of
    a wave, pass it and share its two or three bins); one about the source itself (every ray at s = 0: a whole wave in one bin); one
    across the room."""
    S = np.array([0.31, 0.42, 0.37]) * np.asarray(size)
    d0 = scenes.burst_rays(64, size)[0, 3:]
    c = np.stack([S + 2.0 * d0 / np.sqrt((d0 * d0).sum()), S, np.array([0.8, 0.3, 0.6]) * np.asarray(size)])
    return np.ascontiguousarray(c), np.array([1.0, 0.25, 0.75])


def burst_case(n, B, order, mode="specular", aggregate=1, partition=("voxel", 8), frac_bits=40, seed=5, bounces=4):
    verts, nverts, size = _register()
    P = verts.shape[0]
    rng = np.random.default_rng(7000 + 10 * n + B)
    centers, radii = burst_receivers(size)
    alpha = rc.alpha_table(P, B, rng) if B > 1 else None
    if alpha is not None:
        alpha[:] = np.minimum(alpha, 0.6)                     # 12 polygons: keep every wall reflecting, so four casts stay populated
    sigma = rc.sigma_table(P, B, rng) if mode != "specular" else None
    name = f"burst-n{n}-B{B}-o{order}-{mode}-a{aggregate}-{partition[0]}"
    return AmbiCase(name, SHOEBOX12, partition, scenes.burst_rays(n, size), bounces, centers, radii, 64, 0.5, frac_bits, mode, True, aggregate, 1, alpha,
                    sigma, None, seed, order=order)


def scene_cases():
    """n x B x order, specular, aggregated (tests run each with "receive_aggregate" 0 too: identical bytes)."""
    return [burst_case(n, B, order) for order in (2, 3) for B in BANDS for n in SIZES]


def scatter_cases():
    """Seeded scattering with the rain off and on."""
    return [burst_case(4159, 3, order, mode=mode, seed=77 + order) for order in (2, 3) for mode in ("scatter", "rain")]


def partition_cases():
    return [burst_case(4097, 3, 3, mode="scatter", partition=p) for p in (("voxel", 8), ("octree", 4, 8), ("kdtree", 8, 6))]


# ---- the numeric edges
AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
DIAGONALS = [(1, 1, 0), (1, -1, 0), (-1, 1, 0), (1, 0, 1), (-1, 0, 1), (0, 1, 1), (0, 1, -1), (1, 1, 1), (-1, 1, 1), (1, -1, -1), (-1, -1, -1)]


def aimed_rays(n, center, scale=1.0):
    """n rays through `center` along the axes and the 45-degree diagonals in turn, each from 1.5 of its direction vectors away: the
    arrival vector's components are 0, +-1, +-sqrt(1/2) and +-sqrt(1/3) as the division leaves them, whose products are exact or land
    half way."""
    dirs = np.array(AXES + DIAGONALS, np.float64)
    d = dirs[np.arange(n) % dirs.shape[0]] * scale
    return np.ascontiguousarray(np.concatenate([center - 1.5 * d, d], axis=1))


def edge_case(name, order, frac_bits, n=257, B=5, aggregate=1, special_rays=False, device=False):
    """Axis-aligned and diagonal arrivals at a receiver in the middle of the 972-triangle shoebox, the state from receive_cases'
    edge_state: E from its special values (NaN, +-inf, 0.5, 1.5, 2.5, 2^62, 2^63, 1e300 ...), so that with frac_bits 0 m reaches 2^63 --
    every channel then stands at the +-2^62 clamp, Y6 = -0.5 at z = 0 exactly on it -- and m * Y lands on .5 ties (m = 1, 3, 5 against
    Y6 = -0.5 at frac_bits 0 and 1).  special_rays: beside them, rays with a NaN direction component, an all-zero direction and
    directions scaled by 2^-600 (len = 0): they detect nothing, and their lanes' channels must add 0 to the wave's sums."""
    verts, nverts, size = rc.mesh_of(("shoebox",))
    P = verts.shape[0]
    rng = np.random.default_rng(4242 + 100 * order + frac_bits + n)
    center = np.array([5.0, 3.5, 2.0])
    centers = np.stack([center, center, center + np.array([0.25, 0.0, 0.0])])
    radii = np.array([0.5, 0.125, 1.0])
    rays = aimed_rays(n, center)
    if special_rays:
        rays[5::32, 3] = np.nan
        rays[9::32, 3:] = 0.0
        rays[17::32, 3:] *= rc.TINY
    alpha = rc.alpha_table(P, B, rng)
    state = rc.edge_state(n, B, 64, 0.0625, rng, False)
    state[0, 2::3] = rng.uniform(0.0, 2.0, state[0, 2::3].shape)      # the ordinary rays are binned: 1.5 .. 2.6 m and their start
    state[0, ::6] = 0.0                                                # and half of the special ones start at L = 0: their E is deposited
    return AmbiCase(name, ("shoebox",), ("voxel", 8), rays, 2, centers, radii, 64, 0.0625, frac_bits, "specular", True, aggregate, 1, alpha, None,
                    state, 5, device=device, order=order)


def edge_cases():
    out = []
    for order in (2, 3):
        for frac_bits in (0, 1, 62):
            out.append(edge_case(f"edge-o{order}-f{frac_bits}", order, frac_bits, device=frac_bits == 0))
        for agg in (1, 0):
            out.append(edge_case(f"edge-special-o{order}-a{agg}", order, 0, n=4159, B=8, aggregate=agg, special_rays=True))
    return out


# ---- the sweep
def sweep_case(seed):
    """receive_cases.sweep_case(seed) with directional on and an order drawn from the seed; every third a receiver map over the same
    receivers (never with rain: the library refuses that pair, and so does the reference)."""
    rng = np.random.default_rng(0xA3B10000 + int(seed))
    base = rc.sweep_case(seed)
    order = int(rng.integers(2, 4))
    as_map = int(seed) % 3 == 0 and base.mode != "rain"
    case = with_order(base, order, name=f"ambi-sweep-{seed}", map_cell=0.0 if as_map else None, n_bins=min(base.n_bins, 512),
                      bounces=min(base.bounces, 5))
    assert case.words <= rc.WORDS_MAX
    return case


SWEEP_SEEDS = range(50)


def fixed_cases():
    return scene_cases() + scatter_cases() + partition_cases() + edge_cases()
