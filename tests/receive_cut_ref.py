"""The cases of the termination rules' tests (include/hare_hip.h, "receivers", "Termination"): the time limit
(HARE_RECEIVE_TIME_LIMIT) and the energy floor with optional Russian roulette (scene options "receive_floor_bits", "receive_roulette").
The rules themselves are restated in tests/receive_ref.py (decide, and receive_loop's termination block); here are the fixed set
cut_cases() of tests/test_gpu_receive_cut.py and tests/test_receive_cut_api.py and the seeded sweep_cut_case(seed) -- plain
tests.receive_cases.Case records with the rules set, run by tests.receive_cases.reference like every other case."""
import numpy as np

import hare_amd.scenes as scenes
from tests import receive_cases
from tests.receive_cases import Case, mesh_of, sweep_case


def open_room():
    """The partition room of tests.receive_cases with half of its ceiling taken out: some rays leave and retire by missing."""
    verts, nverts, size = receive_cases.partition_room()
    top = np.array([(verts[i, :nverts[i], 2] == size[2]).all() and verts[i, :nverts[i], 0].min() >= 0.5 * size[0] for i in range(verts.shape[0])])
    assert top.any()
    return np.ascontiguousarray(verts[~top]), np.ascontiguousarray(nverts[~top]), size


OPEN_ROOM = ("room-open",)
receive_cases._MESHES.setdefault(OPEN_ROOM, open_room())       # mesh_of serves it from here on, to the oracle and to the library alike

FLOOR_BITS = 5      # F = 2^-5: with the absorption below the first rays pass under it in cast 4 or 5, the last ones not within 12 casts
RULES = {"time": dict(time_limit=True), "floor": dict(floor_bits=FLOOR_BITS), "roulette": dict(floor_bits=FLOOR_BITS, roulette=True),
         "all": dict(time_limit=True, floor_bits=FLOOR_BITS, roulette=True)}
PARTITIONS = {"voxel": ("voxel", 8), "octree": ("octree", 4, 8), "kdtree": ("kdtree", 8, 6)}
BOUNCES = 12
BIN_LEN = 0.25
N_BINS = 160        # 40 m: about ten mean free paths (4 V / S = 4.06 m in the shoebox).  At six, fewer than 1 % of the rays are left in
                    # cast 11; at ten the limit bites from cast 4 and a third of the rays still run the last cast


def cut_case(name, rule, n, partition="voxel", B=1, mode="specular", directional=False, pack=1, aggregate=1, scene=("shoebox",), device=False,
             special_state=False, seed=11):
    rng = np.random.default_rng(7000 + 10 * n + B)
    verts, nverts, size = mesh_of(scene)
    P = verts.shape[0]
    rays = scenes.burst_rays(n, size)
    S = np.array([0.31, 0.42, 0.37]) * np.asarray(size)
    centers = np.ascontiguousarray(np.stack([S, np.array([0.7, 0.6, 0.5]) * size, np.array([0.2, 0.8, 0.7]) * size]))
    radii = np.array([0.5, 0.9, 0.7])
    # alpha about 0.3 in the mean: half of the polygons near 0.1, half near 0.5, a little apart per band.  The rays' energies spread
    # over decades, so the floor bites from cast 4 or 5 on, not all at once, and leaves rays for the last cast
    alpha = np.where(rng.random((P, 1)) < 0.5, 0.1, 0.5) + rng.uniform(-0.05, 0.05, (P, B))
    sigma = np.full((P, B), 0.3) if mode != "specular" else None
    state = None
    if special_state:
        # L already past the end for every ninth ray, +inf and NaN among them; a few energies under the floor, 0, NaN and inf from the start
        state = np.concatenate([rng.uniform(0.0, 0.15 * N_BINS * BIN_LEN, (1, n)), rng.uniform(0.5, 1.5, (B, n))])
        i = np.arange(n)
        state[0, i % 9 == 0] = np.array([N_BINS * BIN_LEN, 1.5 * N_BINS * BIN_LEN, np.inf, np.nan, 1e300, -np.inf])[(i[i % 9 == 0] // 9) % 6]
        for b in range(B):
            at = i % 7 == b
            state[1 + b, at] = np.array([0.0, -0.0, np.nan, np.inf, 2.0 ** -9, -1.0, 5e-324])[(i[at] // 7) % 7]
    return Case(name, scene, PARTITIONS[partition], rays, BOUNCES, centers, radii, N_BINS, BIN_LEN, 40, mode, directional, aggregate, pack, alpha,
                sigma, state, seed, None, None, 1, device, **RULES[rule])


def cut_cases():
    """The fixed set: each rule alone, the floor with roulette, and all together, at n = 63, 257, 4097 and 4159 (a partial wave, a
    partial workgroup, both sides of the live-block list's threshold); the three partitions; B = 1 and 3; no scattering table (the
    roulette then draws without one), sigma = 0.3, rain; directional; bounce_pack and receive_aggregate 0 / 1; a starting state with L
    past the end, infinities and NaN; an open room in which rays also retire by missing."""
    c = [
        cut_case("time-4159", "time", 4159, device=True),
        cut_case("time-4097", "time", 4097, B=3, mode="scatter", directional=True, pack=0, aggregate=0),
        cut_case("time-257", "time", 257, "octree", B=3, mode="rain"),
        cut_case("time-63", "time", 63, "kdtree", directional=True),
        cut_case("floor-4159", "floor", 4159, B=3, mode="scatter", device=True),
        cut_case("floor-4097", "floor", 4097, "kdtree"),
        cut_case("floor-257", "floor", 257, B=3, mode="rain", directional=True, aggregate=0),
        cut_case("floor-63", "floor", 63, "octree", B=3),
        cut_case("roulette-4159", "roulette", 4159, B=3, device=True),
        cut_case("roulette-4097", "roulette", 4097, "octree", B=3, mode="scatter", directional=True),
        cut_case("roulette-257", "roulette", 257, "kdtree", mode="rain"),
        cut_case("roulette-63", "roulette", 63, B=3, mode="scatter", aggregate=0),
        cut_case("all-4159", "all", 4159, B=3, mode="rain", directional=True, device=True),
        cut_case("all-4097", "all", 4097, pack=0, device=True),
        cut_case("all-257", "all", 257, "octree", B=3, mode="scatter"),
        cut_case("all-63", "all", 63, "kdtree", B=3),
        cut_case("all-state", "all", 4159, B=3, mode="scatter", special_state=True, device=True),
        cut_case("all-open-room", "all", 4159, B=3, scene=OPEN_ROOM, device=True),
        cut_case("time-open-room", "time", 4097, "kdtree", mode="scatter", scene=OPEN_ROOM),
        cut_case("floor-open-room-pack0", "floor", 4159, B=3, pack=0, scene=OPEN_ROOM),
    ]
    names = [x.name for x in c]
    assert len(set(names)) == len(names)
    return c


def sweep_cut_case(seed):
    """tests.receive_cases.sweep_case(seed) with the rules drawn on top, from a generator of their own; nothing is redrawn."""
    rng = np.random.default_rng(0xC0750000 + int(seed))
    return sweep_case(seed).without(time_limit=bool(rng.integers(0, 2)), floor_bits=int(rng.choice([0, 1, 2, 4, 8, 20, 1000])),
                                    roulette=bool(rng.integers(0, 2)))
