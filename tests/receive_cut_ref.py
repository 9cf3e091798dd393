"""numpy restatement of the receive loop WITH its termination rules (include/hare_hip.h, "receivers", "Termination"): the time limit
(HARE_RECEIVE_TIME_LIMIT) and the energy floor with optional Russian roulette (scene options "receive_floor_bits", "receive_roulette"),
operation for operation in FP64.  cut_loop is tests.receive_ref.receive_loop cast by cast, built from that module's and
tests.scatter_ref's functions, with the rules decided behind every cast's state update; with both rules off it returns exactly what
receive_loop returns (tests/test_receive_cut_api.py asserts it).  It also returns, per cast, how many rays were live, how many each rule
retired and how many roulette survivors were boosted.

Below it: the cases of the device tests (tests/test_gpu_receive_cut.py) -- CutCase, a tests.receive_cases.Case with the rules on top --
and reference(), which runs cut_loop on one and keeps the result (the CPU and the device tests share it; nobody changes it)."""
import dataclasses

import numpy as np

import hare_amd.scenes as scenes
from oracle import pyoracle as po
from tests import receive_cases
from tests.receive_cases import Case, mesh_of, oracle_of, sweep_case
from tests.receive_ref import rain_step, receiver_step, side_normals
from tests.scatter_ref import choose, normals_of, ray_base, scatter_rays, uniform, weights

ROULETTE_WORD = 65                       # u_65: scattering draws j = 0 .. 64


def decide(L, E, base, c, n_bins, bin_len, time_limit, floor_bits, roulette):
    """The rules for m rays that hit in cast c and would be reflected: L [m] and E [B, m] AFTER the cast's state update, base [m] the
    RNG's per-ray base.  Returns (cut_time [m] bool, cut_floor [m] bool, boosted [m] bool, E' [B, m]): E' is E but for the roulette's
    survivors, whose bands are divided by ps."""
    m_rays = L.shape[0]
    cut_time = np.zeros(m_rays, bool)
    cut_floor = np.zeros(m_rays, bool)
    boosted = np.zeros(m_rays, bool)
    E = E.copy()
    with np.errstate(all="ignore"):
        if time_limit:
            cut_time = (L / np.float64(bin_len)) >= np.float64(n_bins)          # a NaN compares false
        if floor_bits:
            F = np.ldexp(np.float64(1.0), -int(floor_bits))
            m = E[0].copy()
            for b in range(1, E.shape[0]):
                m = np.where(E[b] > m, E[b], m)                                  # a NaN E[b] never replaces m
            below = (m < F) & ~cut_time                                          # m = NaN: not below
            if roulette:
                at = np.nonzero(below)[0]
                ps = m[at] / F
                u = uniform(base[at], c, ROULETTE_WORD)
                win = u < ps
                E[:, at[win]] = E[:, at[win]] / ps[win]
                boosted[at[win]] = True
                cut_floor[at[~win]] = True
            else:
                cut_floor = below
    return cut_time, cut_floor, boosted, E


def cut_loop(po, topo, part, rays, bounces, centers, radii, n_bins, bin_len, frac_bits, alpha=None, sigma=None, seed=0, state_in=None, g0=0,
             rain=False, directional=False, time_limit=False, floor_bits=0, roulette=False, stats=None, nthreads=16, tallies=None, excl1=None,
             excl2=None, last_events=None):
    """tests.receive_ref.receive_loop with the two rules.  Returns (hist, det, state [1 + B, n], final rays [n, 6], per_cast) with per_cast
    a dict of int64 arrays [bounces]: "live" (rays that took part in the cast), "time" and "floor" (rays the rule retired in it) and
    "boosted" (roulette survivors)."""
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    n = rays.shape[0]
    B = 1
    for t in (alpha, sigma):
        if t is not None:
            B = np.asarray(t).shape[1]
    K = np.asarray(centers).reshape(-1, 3).shape[0]
    hist = np.zeros((K, n_bins, B, 4) if directional else (K, n_bins, B), np.uint64)
    det = np.zeros((K, 2), np.uint64)
    if state_in is None:
        L, E = np.zeros(n), np.ones((B, n))
    else:
        st = np.array(state_in, np.float64).reshape(1 + B, n)
        L, E = st[0].copy(), st[1:].copy()
    normals = normals_of(topo)
    base = ray_base(seed, np.arange(g0, g0 + n, dtype=np.uint64))
    cur = rays.copy()
    e1 = np.full(n, -1, np.int32) if excl1 is None else np.asarray(excl1, np.int32).copy()
    e2 = None if excl2 is None else np.asarray(excl2, np.int32).copy()
    live = np.ones(n, bool)
    rained = np.zeros(n, bool)
    per_cast = {k: np.zeros(bounces, np.int64) for k in ("live", "time", "floor", "boosted")}
    for c in range(bounces):
        per_cast["live"][c] = int(live.sum())
        ev = np.zeros(n, po.XEVENT_DTYPE)
        ev["poly_id"] = -1
        if live.any():
            ev[live] = part.shoot(cur[live], excl1=e1[live], excl2=None if e2 is None else e2[live], nthreads=nthreads)[0]
        hit = ev["hit"] == 1
        t_end = np.where(hit, ev["t"], np.inf)
        seen = live & ~rained
        if seen.any():
            receiver_step(cur[seen, :3], cur[seen, 3:], t_end[seen], L[seen], E[:, seen], centers, radii, n_bins, bin_len, frac_bits, hist, det,
                          None, tallies)
        upd = live & hit
        if alpha is not None:
            a = np.asarray(alpha, np.float64)[ev["poly_id"][upd]].T
            with np.errstate(invalid="ignore"):
                E[:, upd] = E[:, upd] * (1.0 - a)
        L[upd] = L[upd] + ev["t"][upd]
        rained = np.zeros(n, bool)
        goes_on = upd
        if c + 1 < bounces:
            nxt = po.reflect_batch(topo, cur, ev)
            idx = np.nonzero(upd)[0]
            if sigma is not None and idx.size:
                pid = ev["poly_id"][idx]
                srow = np.asarray(sigma, np.float64)[pid]
                p, diff = choose(srow, uniform(base[idx], c, 0))
                if rain:
                    t = p > 0
                    ti = idx[t]
                    if ti.size:
                        d = cur[ti, 3:]
                        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
                        x = np.stack([ev["x"][ti], ev["y"][ti], ev["z"][ti]], axis=1)
                        rain_step(part, x, side_normals(d, normals[pid[t]]), pid[t], length, L[ti], E[:, ti], srow[t].T, centers, radii, n_bins,
                                  bin_len, frac_bits, hist, det, stats=stats, nthreads=nthreads, tallies=tallies)
                    rained[idx[diff]] = True
                with np.errstate(invalid="ignore", over="ignore"):
                    E[:, idx] = E[:, idx] * weights(srow, p, diff).T
                di = idx[diff]
                if di.size:
                    nxt[di] = scatter_rays(cur[di], ev[di], normals, base[di], c)
            # ---- termination: behind the state update; a retired ray keeps the ray the cast received and is treated as a miss from here
            if (time_limit or floor_bits) and idx.size:
                ct, cf, boosted, E[:, idx] = decide(L[idx], E[:, idx], base[idx], c, n_bins, bin_len, time_limit, floor_bits, roulette)
                gone = idx[ct | cf]
                nxt[gone] = cur[gone]
                goes_on = upd.copy()
                goes_on[gone] = False
                rained[gone] = False
                for name, v in (("time", ct), ("floor", cf), ("boosted", boosted)):
                    per_cast[name][c] = int(v.sum())
            cur = nxt
        e1 = np.where(goes_on, ev["poly_id"], -2).astype(np.int32)
        e2 = None
        live = goes_on
        if last_events is not None and c + 1 == bounces:
            last_events.append(ev)
    return hist, det, np.concatenate([L[None], E], axis=0), cur, per_cast


def same_bits(got, want):
    """None when the two arrays agree: NaN where the other has NaN (its sign and payload are the FPU's), the same bits everywhere else.
    Otherwise the first differences, as text."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape / dtype {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        bad = (gn != wn) | (~gn & ~wn & (got.view(np.int64) != want.view(np.int64)))
    else:
        bad = got != want
    if bad.any():
        at = np.argwhere(bad)[:4]
        return f"{int(bad.sum())} differ, first at {at.tolist()}: got {[got[tuple(i)] for i in at]} want {[want[tuple(i)] for i in at]}"
    return None


# ---- cases
@dataclasses.dataclass
class CutCase:
    case: Case
    time_limit: bool = False
    floor_bits: int = 0
    roulette: bool = False

    @property
    def name(self):
        return self.case.name

    def describe(self):
        return f"{self.case.describe()} time_limit={int(self.time_limit)} floor_bits={self.floor_bits} roulette={int(self.roulette)}"

    def without(self, **rules):
        return dataclasses.replace(self, **rules)


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
    case = Case(name, scene, PARTITIONS[partition], rays, BOUNCES, centers, radii, N_BINS, BIN_LEN, 40, mode, directional, aggregate, pack, alpha,
                sigma, state, seed, None, None, 1, device)
    return CutCase(case, **RULES[rule])


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
    return CutCase(sweep_case(seed), bool(rng.integers(0, 2)), int(rng.choice([0, 1, 2, 4, 8, 20, 1000])), bool(rng.integers(0, 2)))


_REFERENCES = {}


def reference(cc, nthreads=16, keep=True):
    """cut_loop on the case: dict of hist, det, state, rays, events (the last cast's), per_cast, stats and tallies.  Kept by the case's
    name and rules (the tests share it and leave it unchanged)."""
    key = (cc.name, cc.time_limit, cc.floor_bits, cc.roulette)
    if key in _REFERENCES:
        return _REFERENCES[key]
    case = cc.case
    To, o = oracle_of(case)
    stats, tallies, last = {}, {}, []
    hist, det, state, rays, per_cast = cut_loop(po, To, o, case.rays, case.bounces, case.centers, case.radii, case.n_bins, case.bin_len,
                                                case.frac_bits, alpha=case.alpha, sigma=case.sigma if case.mode != "specular" else None,
                                                seed=case.seed, state_in=case.state_in, rain=case.mode == "rain", directional=case.directional,
                                                time_limit=cc.time_limit, floor_bits=cc.floor_bits, roulette=cc.roulette, stats=stats,
                                                nthreads=nthreads, tallies=tallies, excl1=case.excl1, excl2=case.excl2, last_events=last)
    out = dict(hist=hist, det=det, state=state, rays=rays, events=last[0], per_cast=per_cast, stats=stats, tallies=tallies)
    if keep:
        _REFERENCES[key] = out
    return out
