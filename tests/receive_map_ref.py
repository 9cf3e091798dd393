"""numpy restatement of receiver maps (include/hare_hip.h, "receivers", "Receiver maps"), operation for operation in FP64: the grid the
setter builds (build_grid: cells, CSR) and the visit rule as a candidate mask per ray and cast (candidates).  The loop is
tests.receive_ref.receive_loop with visit=functools.partial(candidates, grid): its receiver step then runs, per receiver, on the rays
that hold the receiver as a candidate (a map refuses the rain).

Below it: the cases that the CPU tests (tests/test_receive_map_api.py) and the device tests (tests/test_gpu_receive_map.py) share --
plain tests.receive_cases.Case records with map_cell set, run by tests.receive_cases.reference like every other case.  Then the cases
at the visit rule's edges (map_edge_cases) and a seeded sweep (map_sweep_case), for tests/test_receive_map_cases.py (no GPU) and
tests/test_gpu_receive_map_{edges,sweep}.py; candidates() counts the classes of the rule a call went through (MAP_TALLIES)."""
import dataclasses

import numpy as np

import hare_amd.scenes as scenes
from oracle import pyoracle as po
from tests.receive_cases import TINY, Case, edge_state, mesh_of

MAX_CELLS = 1 << 21
MAX_K = 65536
F = np.float64


@dataclasses.dataclass
class Grid:
    origin: np.ndarray          # lo_a
    h: float                    # cell edge
    R: float                    # r_max + h / 8
    pad: float                  # P = R / h
    dims: np.ndarray            # n_a (int64)
    cell_of: np.ndarray         # [K, 3] the cell of every receiver's center
    cell_start: np.ndarray      # [cells + 1] uint32
    cell_items: np.ndarray      # [K] uint32, ascending k within a cell

    @property
    def cells(self):
        return int(self.dims.prod())


def _idx(x, n):
    """idx(x, n) of the header for floor'd doubles x: clamped as doubles to 0 .. n - 1, NaN -> 0, then converted."""
    x = np.asarray(x, F)
    return np.where(x >= 0, np.where(x < F(n), x, F(n - 1)), F(0)).astype(np.int64)


def build_grid(centers, radii, cell=0.0):
    c = np.ascontiguousarray(centers, F).reshape(-1, 3)
    r = np.ascontiguousarray(radii, F).reshape(-1)
    with np.errstate(all="ignore"):
        r_max = F(r.max())
        lo, hi = c.min(axis=0), c.max(axis=0)
        h = F(cell) if cell > 0 else F(2.0) * r_max
        while True:
            n = []
            for a in range(3):
                q = (hi[a] - lo[a]) / h
                n.append(int(np.floor(q)) + 1 if (q >= 0 and q < F(MAX_CELLS)) else (1 if q != q else MAX_CELLS + 1))
            if n[0] * n[1] * n[2] <= MAX_CELLS:
                break
            h = h * F(2.0)
        R = r_max + h / F(8.0)
        pad = R / h
        dims = np.array(n, np.int64)
        u = (c - lo[None, :]) / h
        cell_of = np.stack([_idx(np.floor(u[:, a]), n[a]) for a in range(3)], axis=1)
    lin = (cell_of[:, 2] * dims[1] + cell_of[:, 1]) * dims[0] + cell_of[:, 0]
    start = np.zeros(int(dims.prod()) + 1, np.uint32)
    start[1:] = np.cumsum(np.bincount(lin, minlength=int(dims.prod())))
    items = np.argsort(lin, kind="stable").astype(np.uint32)
    return Grid(lo.copy(), float(h), float(R), float(pad), dims, cell_of, start, items)


MAP_TALLIES = ("axis1", "axis2", "face_lo", "face_hi", "clip_nan", "tie_major_same", "tie_major_opposite", "enter", "leave", "touch",
               "half_line", "clamp_lo_slab", "clamp_hi_slab", "clamp_nan_slab", "clamp_lo_range", "clamp_hi_range", "clamp_nan_range",
               "slab_skipped", "pad_only", "pad_only_major0", "pad_only_major1", "pad_only_major2", "pad_only_minor0", "pad_only_minor1",
               "pad_only_minor2", "end_slab", "lost", "detected")


# the per-ray classes a detection can hang on; <name>_det counts the rays of the class that hold at least one detected candidate
RAY_CLASSES = ("axis1", "axis2", "tie_major_same", "tie_major_opposite", "enter", "leave", "half_line", "clamp_lo_slab", "clamp_hi_slab")
DET_TALLIES = tuple(name + "_det" for name in RAY_CLASSES)


def _count(tallies, name, mask):
    tallies[name] = tallies.get(name, 0) + int(np.count_nonzero(mask))


def _clamps(tallies, where, x, n, rows=None):
    """The idx() calls on the floor'd doubles x that clamped below 0, at n, or took a NaN (where: "slab" or "range")."""
    if tallies is None:
        return
    x = x if rows is None else x[rows]
    _count(tallies, "clamp_lo_" + where, x < 0)
    _count(tallies, "clamp_hi_" + where, x >= F(n))
    _count(tallies, "clamp_nan_" + where, x != x)


SLABS_COUNTED = 256                      # a ray of at most this many slabs has every slab of jlo .. jhi tested for slab_skipped


def _skipped(tallies, jlo, jhi, um, vm, t0, t1, P):
    """slab_skipped of the rays given, over EVERY slab j = jlo .. jhi (rays of at most SLABS_COUNTED slabs), by the rule's own operations."""
    few = (jhi - jlo) < SLABS_COUNTED
    jlo, jhi, um, vm, t0, t1 = (x[few] for x in (jlo, jhi, um, vm, t0, t1))
    for k in range(int((jhi - jlo).max(initial=-1)) + 1):
        fj = (jlo + k).astype(F)
        tA = ((fj - P) - um) / vm
        tB = (((fj + F(1.0)) + P) - um) / vm
        tlo, thi = np.where(tA < tB, tA, tB), np.where(tA < tB, tB, tA)
        ts, te = np.where(tlo > t0, tlo, t0), np.where(thi < t1, thi, t1)
        _count(tallies, "slab_skipped", (jlo + k <= jhi) & ~(ts <= te))
    return few


def linear_detected(o, d, t_end, centers, radii):
    """bool [m, K]: the (ray, receiver) pairs that tests.receive_ref.receiver_step detects with every receiver visited -- its test, in
    its order of operations, for all pairs at once (tests/test_receive_map_cases.py holds the two together)."""
    c = np.asarray(centers, F).reshape(-1, 3)
    r2 = np.asarray(radii, F) * np.asarray(radii, F)
    out = np.zeros((o.shape[0], c.shape[0]), bool)
    ox, oy, oz, dx, dy, dz = (x[:, None] for x in (o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]))
    step = max(1, (1 << 21) // max(1, o.shape[0]))
    with np.errstate(all="ignore"):
        dd = (dx * dx + dy * dy) + dz * dz
        for k0 in range(0, c.shape[0], step):
            cx, cy, cz = (c[None, k0:k0 + step, a] for a in range(3))
            wx, wy, wz = cx - ox, cy - oy, cz - oz
            s = ((wx * dx + wy * dy) + wz * dz) / dd
            qx, qy, qz = (ox + dx * s) - cx, (oy + dy * s) - cy, (oz + dz * s) - cz
            out[:, k0:k0 + step] = (s >= 0) & (s < t_end[:, None]) & (((qx * qx + qy * qy) + qz * qz) < r2[None, k0:k0 + step])
    return out


def candidates(g, o, d, t_end, tallies=None, centers=None, radii=None):
    """The visit rule: bool [m, K], True where the cell of receiver k is visited by ray i (o, d [m, 3]; t_end [m], +inf for a miss).
    tallies (dict, optional) collects how often the call went through each class of the rule (MAP_TALLIES), as `tallies` of
    tests.receive_ref.deposit does; the mask does not depend on it.  Per ray: axis1 / axis2 (exactly one / two v_a == 0, clip passed);
    tie_major_same / _opposite (|v_1| == |v_0| or |v_2| == |v_m|, not zero, by the signs; clip passed); enter (t0 > 0), leave
    (t1 < t_end), touch (t0 == t1), half_line (t_end == +inf), each of a ray with candidates allowed.  Per ray and axis: face_lo / face_hi
    (v_a == 0 with u_a == L / == H), clip_nan.  Per idx() call: clamp_lo / clamp_hi / clamp_nan, for the slab range (_slab) and for the
    other two axes (_range), over the slabs that hold a receiver, the ones this restatement evaluates; slab_skipped over every slab of
    jlo .. jhi for a ray of at most SLABS_COUNTED slabs, over the slabs that hold a receiver for a longer one.  With
    centers and radii given, per (ray, receiver): detected (a candidate that linear_detected detects); pad_only (a detected candidate
    whose cell is outside the ranges its slab gives with P taken as 0 in the ranges and in jlo / jhi; _major<a>: it is the slab range
    that misses it, _minor<a>: the range of the axis a); end_slab (a detected candidate in slab jlo or jhi of a ray of at least 3
    slabs); lost (detected by linear_detected and not a candidate); and <class>_det for the per-ray classes of RAY_CLASSES: the rays of
    the class that hold at least one detected candidate (clamp_*_slab_det: rays whose jlo / jhi clamped)."""
    o = np.asarray(o, F).reshape(-1, 3)
    d = np.asarray(d, F).reshape(-1, 3)
    t_end = np.asarray(t_end, F).reshape(-1)
    m_rays, K = o.shape[0], g.cell_of.shape[0]
    h, P = F(g.h), F(g.pad)
    cand = np.zeros((m_rays, K), bool)
    with np.errstate(all="ignore"):
        u = (o - g.origin[None, :]) / h
        v = d / h
        t0, t1, ok = np.zeros(m_rays), t_end.copy(), np.ones(m_rays, bool)
        zeros = np.zeros(m_rays, np.int64)
        faces, nans = [], []
        for a in range(3):
            L, H = -P, F(g.dims[a]) + P
            z = v[:, a] == 0
            ok &= np.where(z, (u[:, a] >= L) & (u[:, a] <= H), True)
            ta = (L - u[:, a]) / v[:, a]
            tb = (H - u[:, a]) / v[:, a]
            ok &= np.where(z, True, (ta == ta) & (tb == tb))
            tmin, tmax = np.where(ta < tb, ta, tb), np.where(ta < tb, tb, ta)
            t0 = np.where(~z & (tmin > t0), tmin, t0)
            t1 = np.where(~z & (tmax < t1), tmax, t1)
            zeros += z
            faces.append((z & (u[:, a] == L), z & (u[:, a] == H)))
            nans.append(~z & ~((ta == ta) & (tb == tb)))
        ok &= (t0 <= t1) & (t1 < np.inf)
        major = np.zeros(m_rays, np.int64)
        vm = v[:, 0].copy()
        ties = []
        for a in (1, 2):
            ties.append(((np.abs(v[:, a]) == np.abs(vm)) & ~(vm == 0), np.signbit(v[:, a]) == np.signbit(vm)))
            big = np.abs(v[:, a]) > np.abs(vm)
            major = np.where(big, a, major)
            vm = np.where(big, v[:, a], vm)
        ray = {}                                      # the per-ray classes, as masks [m]
        if tallies is not None:
            ray["axis1"], ray["axis2"] = ok & (zeros == 1), ok & (zeros == 2)
            ray["tie_major_same"] = ok & ((ties[0][0] & ties[0][1]) | (ties[1][0] & ties[1][1]))
            ray["tie_major_opposite"] = ok & ((ties[0][0] & ~ties[0][1]) | (ties[1][0] & ~ties[1][1]))
            _count(tallies, "axis1", ray["axis1"])
            _count(tallies, "axis2", ray["axis2"])
            for lo_face, hi_face in faces:
                _count(tallies, "face_lo", lo_face)
                _count(tallies, "face_hi", hi_face)
            for bad in nans:
                _count(tallies, "clip_nan", bad)
            for tie, same in ties:
                _count(tallies, "tie_major_same", ok & tie & same)
                _count(tallies, "tie_major_opposite", ok & tie & ~same)
        ok &= ~(vm == 0)
        um = u[np.arange(m_rays), major]
        a0, a1 = um + vm * t0, um + vm * t1
        amin, amax = np.where(a0 < a1, a0, a1), np.where(a0 < a1, a1, a0)
        if tallies is not None:
            ray.update(enter=ok & (t0 > 0), leave=ok & (t1 < t_end), touch=ok & (t0 == t1), half_line=ok & (t_end == np.inf),
                       clamp_lo_slab=ok & (np.floor(amin - P) < 0), clamp_hi_slab=ok & (np.floor(amax + P) >= g.dims[major].astype(F)))
            for name in ("enter", "leave", "touch", "half_line"):
                _count(tallies, name, ray[name])
        pairs = tallies is not None and centers is not None
        if pairs:                                     # the visit with P taken as 0 in the ranges and in jlo / jhi, per axis
            in0 = [np.zeros((m_rays, K), bool) for _ in range(3)]
            jlo_all, jhi_all = np.zeros(m_rays, np.int64), np.zeros(m_rays, np.int64)
        for mm in range(3):
            rows = np.nonzero(ok & (major == mm))[0]
            if rows.size == 0:
                continue
            nm = int(g.dims[mm])
            jlo, jhi = _idx(np.floor(amin[rows] - P), nm), _idx(np.floor(amax[rows] + P), nm)
            _clamps(tallies, "slab", np.floor(amin[rows] - P), nm)
            _clamps(tallies, "slab", np.floor(amax[rows] + P), nm)
            if tallies is not None:
                few = _skipped(tallies, jlo, jhi, um[rows], vm[rows], t0[rows], t1[rows], P)
            if pairs:
                jlo_all[rows], jhi_all[rows] = jlo, jhi
                jlo0, jhi0 = _idx(np.floor(amin[rows]), nm), _idx(np.floor(amax[rows]), nm)
            others = [a for a in range(3) if a != mm]
            for j in np.unique(g.cell_of[:, mm]):
                ks = np.nonzero(g.cell_of[:, mm] == j)[0]
                at = (jlo <= j) & (j <= jhi)
                rr = rows[at]
                if rr.size == 0:
                    continue
                fj = F(j)
                tA = ((fj - P) - um[rr]) / vm[rr]
                tB = (((fj + F(1.0)) + P) - um[rr]) / vm[rr]
                tlo, thi = np.where(tA < tB, tA, tB), np.where(tA < tB, tB, tA)
                ts = np.where(tlo > t0[rr], tlo, t0[rr])
                te = np.where(thi < t1[rr], thi, t1[rr])
                inside = (ts <= te)[:, None] & np.ones((1, ks.size), bool)
                if tallies is not None:
                    _count(tallies, "slab_skipped", ~(ts <= te) & ~few[at])          # the longer rays: over the slabs that hold a receiver
                if pairs:
                    in0[mm][np.ix_(rr, ks)] = ((jlo0[at] <= j) & (j <= jhi0[at]))[:, None]
                for a in others:
                    p0, p1 = u[rr, a] + v[rr, a] * ts, u[rr, a] + v[rr, a] * te
                    pmin, pmax = np.where(p0 < p1, p0, p1), np.where(p0 < p1, p1, p0)
                    lo_a, hi_a = _idx(np.floor(pmin - P), int(g.dims[a])), _idx(np.floor(pmax + P), int(g.dims[a]))
                    ca = g.cell_of[ks, a][None, :]
                    inside &= (lo_a[:, None] <= ca) & (ca <= hi_a[:, None])
                    _clamps(tallies, "range", np.floor(pmin - P), int(g.dims[a]), ts <= te)
                    _clamps(tallies, "range", np.floor(pmax + P), int(g.dims[a]), ts <= te)
                    if pairs:
                        lo_0, hi_0 = _idx(np.floor(pmin), int(g.dims[a])), _idx(np.floor(pmax), int(g.dims[a]))
                        in0[a][np.ix_(rr, ks)] = (lo_0[:, None] <= ca) & (ca <= hi_0[:, None])
                cand[np.ix_(rr, ks)] = inside
        if pairs:
            det = linear_detected(o, d, t_end, centers, radii)
            hit = det & cand
            _count(tallies, "detected", hit)
            for name in RAY_CLASSES:                  # ... of rays that hold a detection
                _count(tallies, name + "_det", ray[name] & hit.any(axis=1))
            _count(tallies, "lost", det & ~cand)
            _count(tallies, "pad_only", hit & ~(in0[0] & in0[1] & in0[2]))
            for a in range(3):
                is_major = (major == a)[:, None]
                _count(tallies, f"pad_only_major{a}", hit & ~in0[a] & is_major)
                _count(tallies, f"pad_only_minor{a}", hit & ~in0[a] & ~is_major)
            js = np.ascontiguousarray(g.cell_of.T.astype(np.int32))[major]              # [m, K]: the slab of receiver k on ray i's major axis
            ends = ((js == jlo_all[:, None]) | (js == jhi_all[:, None])) & ((jhi_all - jlo_all) >= 2)[:, None]
            _count(tallies, "end_slab", hit & ends)
    return cand


def candidates_tie_high(g, o, d, t_end, tallies=None, centers=None, radii=None):
    """NOT the header's rule: the visit rule with a tie of the major axis given to the HIGHEST axis.  It is candidates() on the problem
    with its axes reversed (x <-> z): every operation of the rule is per axis but the tie-break, and the receivers keep their indices.
    tests/test_receive_map_cases.py uses it to show that the tie-break changes candidates and no result."""
    back = g.cell_of[:, ::-1]
    rev = Grid(g.origin[::-1].copy(), g.h, g.R, g.pad, g.dims[::-1].copy(), np.ascontiguousarray(back), g.cell_start, g.cell_items)
    return candidates(rev, np.asarray(o, F).reshape(-1, 3)[:, ::-1], np.asarray(d, F).reshape(-1, 3)[:, ::-1], t_end)


# ---- map layouts
def map_layout(shape, K, size, rng):
    """(centers [K, 3], radii [K], cell) of one of the map shapes.  plane: a square lattice at z = 1.2 that reaches past the model's
    walls; cloud: points about the model, a fifth of them outside; coincident: a cloud half of whose centers repeat a few points, the
    burst's source among them; big: a cloud with one radius far above the rest; onecell: a cloud under a caller's cell that holds it all;
    cell: a plane under a caller's cell below its receivers' diameter."""
    size = np.asarray(size, F)
    cell = 0.0
    if shape in ("plane", "cell"):
        side = int(np.ceil(np.sqrt(K)))
        span = 1.2 * size[:2]
        step = span / side
        ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="xy"), axis=-1).reshape(-1, 2)[:K]
        centers = np.concatenate([-0.1 * size[:2] + (ij + 0.5) * step, np.full((K, 1), 1.2)], axis=1)
        radii = np.full(K, 0.4 * float(step.min()))
        if shape == "cell":
            cell = 1.3 * float(radii[0])
    else:
        centers = rng.uniform(-0.2, 1.2, (K, 3)) * size
        radii = rng.uniform(0.05, 0.3, K)
        if shape == "coincident":
            pts = np.concatenate([[np.array([0.31, 0.42, 0.37]) * size], rng.uniform(0.2, 0.8, (3, 3)) * size])
            at = np.arange(K) % 2 == 0
            centers[at] = pts[(np.arange(K)[at] // 2) % 4]
        elif shape == "big":
            radii[K // 2] = 2.0
        elif shape == "onecell":
            cell = 100.0
    return np.ascontiguousarray(centers), np.ascontiguousarray(radii), cell


# ---- cases
PARTITIONS = {"voxel": ("voxel", 8), "octree": ("octree", 4, 8), "kdtree": ("kdtree", 8, 6)}
SOUP = ("soup", 120, 40, 3)
N_BINS, BIN_LEN = 48, 0.25          # 12 m: the second and third casts of a 10 m room run past the end (detections that are not binned)


def map_case(name, shape, K, n, B=1, bounces=3, mode="specular", directional=False, partition="voxel", scene=("shoebox",), special=False,
             tiny=False, call="batch", n_bins=N_BINS, rules=None, state=None):
    """call: "batch" (Receive_batch alone), "device" (also receive_device) or "sharded" (also the sharded call over two scenes)."""
    rng = np.random.default_rng(90000 + 7 * K + n)
    verts, nverts, size = mesh_of(scene)
    P = verts.shape[0]
    rays = scenes.burst_rays(n, size) if scene[0] != "soup" else scenes.random_rays(n, size, seed=K + n)
    if tiny:
        rays[17::64, 3:] *= TINY
    centers, radii, cell = map_layout(shape, K, size, rng)
    if K == 1:                            # the one receiver about the burst's source: every ray starts inside it
        centers[0], radii[0] = np.array([0.31, 0.42, 0.37]) * np.asarray(size), 2.5
    alpha = rng.uniform(0.05, 0.5, (P, B)) if B > 1 or K % 2 == 0 else None
    sigma = rng.uniform(0.0, 1.0, (P, B)) if mode != "specular" else None
    state_in = None
    if special:
        state_in = edge_state(n, B, n_bins, BIN_LEN, rng, spread=False)
    elif state or (state is None and bounces == 1):
        state_in = np.concatenate([rng.uniform(-0.5 * BIN_LEN, 1.3 * n_bins * BIN_LEN, (1, n)), rng.uniform(0.0, 2.0, (B, n))])
    return Case(name, scene, PARTITIONS[partition], np.ascontiguousarray(rays), bounces, centers, radii, n_bins, BIN_LEN, 30, mode, directional, 1, 1,
                alpha, sigma, state_in, 1234 + K, None, None, 1, call == "device", map_cell=cell, map_shape=shape, two_scenes=call == "sharded",
                **(rules or {}))


def map_cases():
    """The fixed set: K = 1, 256, 257, 1000, 4096 and one 65 536 with few bins; n = 1, 63, 65, 257, 4097; B = 1, 3, 8; 1 to 4 casts; the four
    kernel forms; the three partitions; shoebox, partition room and an open soup (misses as half-lines); the six map shapes; two cases
    whose states hold the special values of tests.receive_cases and whose rays hold directions scaled by 2^-600; the time limit and the
    floor with roulette; a subset through receive_device, the sharded call and hare_receive_source."""
    c = [
        map_case("K1-n1", "cloud", 1, 1, bounces=4),
        map_case("K1-n65", "onecell", 1, 65, B=3, bounces=3, directional=True, partition="octree", call="device"),
        map_case("K256-plane", "plane", 256, 4097, B=3, bounces=4, call="device"),
        map_case("K257-plane-scatter", "plane", 257, 257, B=8, bounces=3, mode="scatter", partition="kdtree", scene=("room",)),
        map_case("K257-cloud-dir", "cloud", 257, 4097, bounces=2, directional=True, call="sharded"),
        map_case("K1000-cell", "cell", 1000, 4097, B=3, bounces=3, mode="scatter", directional=True, scene=("room",), call="device"),
        map_case("K1000-coincident", "coincident", 1000, 63, B=8, bounces=4, partition="octree"),
        map_case("K4096-plane", "plane", 4096, 4097, bounces=3, partition="kdtree", call="sharded"),
        map_case("K4096-cloud-soup", "cloud", 4096, 257, B=3, bounces=2, mode="scatter", scene=SOUP, state=True),
        map_case("K4096-big", "big", 4096, 65, B=1, bounces=4, directional=True, scene=SOUP, partition="octree", state=True),
        map_case("K256-onecell", "onecell", 256, 257, B=3, bounces=1, mode="scatter", directional=True),
        map_case("K65536-plane", "plane", 65536, 257, bounces=2, n_bins=4, state=True),
        map_case("special-omni", "plane", 1000, 4097, B=3, bounces=2, special=True, tiny=True, call="device"),
        map_case("special-dir", "coincident", 257, 257, B=8, bounces=2, directional=True, special=True, tiny=True, partition="kdtree"),
        map_case("time-limit", "plane", 1000, 4097, B=3, bounces=4, mode="scatter", rules=dict(time_limit=True)),
        map_case("floor-roulette", "cloud", 1000, 4097, B=3, bounces=4, directional=True, rules=dict(floor_bits=2, roulette=True), call="sharded"),
    ]
    names = [x.name for x in c]
    assert len(set(names)) == len(names)
    return c


def identity_cases():
    """K <= 256 receivers that both setters take: the map and the linear loop must give the same bytes."""
    return [map_case("identity-omni", "plane", 256, 4097, B=3, bounces=4),
            map_case("identity-dir", "cloud", 200, 4097, B=3, bounces=3, directional=True, partition="octree"),
            map_case("identity-scatter", "coincident", 256, 4097, B=8, bounces=3, mode="scatter", scene=("room",)),
            map_case("identity-scatter-dir", "cell", 255, 257, B=1, bounces=4, mode="scatter", directional=True, partition="kdtree")]


# ---- the visit rule's edges (tests/test_receive_map_cases.py, tests/test_gpu_receive_map_edges.py)
EXACT_ROOM = ("box", 1.25, 1.0, 1.0, 0.0, 0.0, 0.0)          # 12.5 x 7 x 4 m
# This module's own list: every value of the `special` array inside tests/test_gpu_parity.py::degenerate_rays (a local of that function,
# so it is restated here, in its order), the constants 1e-320, 1e300 and 1e-300 of its `base` rows, and 5e-324, the smallest denormal.
SPECIAL = (0.0, -0.0, 1.0, -1.0, 1e-310, -1e-310, 1e200, np.nan, np.inf, -np.inf, 0.5, 1e-320, 1e300, 1e-300, 5e-324)
EXPECT = {}                              # case name -> the MAP_TALLIES classes the case is there for (each must be > 0)
OUTSIDE = set()                          # names of the cases outside the header's domain


def exact_layout():
    """h = 1 and P = 0.625 exactly: radii 0.5, the default cell, centers on the integers 1 .. 10 x 1 .. 5 x 1 .. 2 (K = 100,
    lo = (1, 1, 1), n = (10, 5, 2)); in EXACT_ROOM the padded faces 0.375 and 11.625 / 6.625 / 3.625 lie inside the walls."""
    c = np.stack(np.meshgrid(np.arange(1.0, 11.0), np.arange(1.0, 6.0), np.arange(1.0, 3.0), indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(c), np.full(c.shape[0], 0.5)


def _beyond(x, lo, face, sign):
    """The double nearest to x, on the side `sign`, whose u = (x - lo) / 1.0 is strictly beyond the face."""
    while not ((x - lo) * sign > face * sign):
        x = np.nextafter(x, sign * np.inf)
    return float(x)


def axis_rays():
    """Axis-parallel rays about the exact layout: along one axis through receivers (two v_a == 0), in a coordinate plane (one), and
    with the zero axes exactly on the padded faces u_a == -P and u_a == n_a + P, and one ulp beyond them."""
    r = [[0.5, 2.25, 1.25, 1, 0, 0], [12.0, 3.25, 1.75, -1, 0, 0], [3.25, 0.5, 1.75, 0, 1, 0], [4.25, 2.75, 0.2, 0, 0, 1], [7.25, 6.5, 1.25, 0, -1, 0],
         [4.25, 2.75, 3.9, 0, 0, -1], [0.5, 1.1, 1.25, 1, 0.5, 0], [0.5, 2.1, 0.3, 1, 0, 0.25], [3.1, 0.5, 0.3, 0, 1, 0.5], [11.9, 4.9, 1.75, -1, -0.5, 0]]
    faces = {0: (0.375, 11.625), 1: (0.375, 6.625), 2: (0.375, 3.625)}
    Hs = {0: 10.625, 1: 5.625, 2: 2.625}
    for a in range(3):
        for along in (b for b in range(3) if b != a):
            for side in (0, 1):
                o = np.array([2.25, 2.25, 1.25])
                o[along] = 0.5
                o[a] = faces[a][side]
                d = np.zeros(3)
                d[along] = 1.0
                r.append(list(o) + list(d))                                   # on the face: two zero axes, one of them on it
                d2 = d.copy()
                d2[3 - a - along] = 0.25
                r.append(list(o) + list(d2))                                  # ... and with one zero axis
                o2 = o.copy()
                o2[a] = _beyond(o[a], 1.0, -0.625 if side == 0 else Hs[a], -1.0 if side == 0 else 1.0)
                r.append(list(o2) + list(d))                                  # one ulp outside: no candidates
    r.append([0.5, 0.375, 3.625, 1, 0, 0])                                    # both zero axes on a face
    return np.array(r, F)


def tie_rays():
    """Ties of the major axis, both signs: (+-1, +-1, +-1), (1, -1, 0), (0, 1, -1) and their kin, each passing receiver (5, 3, 2)."""
    c = np.array([5.0, 3.0, 2.0])
    ds = [[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    ds += [[1, -1, 0], [0, 1, -1], [-1, 1, 0], [0, -1, 1], [1, 1, 0], [0, 1, 1], [1, 0, -1], [1, 0, 1], [2, -2, 1], [1, 2, -2], [0.5, 0.25, 0.5]]
    return np.array([list(c - 0.9 * np.array(d, F) + np.array([0.1, 0.0, 0.05])) + d for d in ds], F)


def pad_rays():
    """Rays that detect receiver (5, 3, 2) without entering its cell: for each ordered pair of axes (A, B), along A with the B
    coordinate 0.05 below the center's (the receiver lies in the next row of a minor axis), and running away from the center's slab
    from a start 0.044 cells short of it, tilted towards B (the receiver lies in the next slab of the major axis)."""
    c = np.array([5.0, 3.0, 2.0])
    r = []
    for A in range(3):
        for B in (b for b in range(3) if b != A):
            C = 3 - A - B
            o, d = c.copy(), np.zeros(3)
            o[B] -= 0.05
            o[C] += 0.1
            o[A] = 0.5
            d[A] = 1.0
            r.append(list(o) + list(d))
            d = np.zeros(3)
            d[A], d[B] = -1.0, 0.1
            p = c.copy()
            p[A] -= 0.045
            p[B] -= 0.45
            r.append(list(p - 0.001 * d) + list(d))
    return np.array(r, F)


def end_rays():
    """Rays across all ten slabs of the x axis that pass the receivers of the first and of the last slab."""
    return np.array([[0.5, 3.1, 1.1, 1, 0, 0], [12.0, 2.1, 1.9, -1, 0, 0], [0.5, 1.2, 1.1, 1, 0.05, 0], [12.2, 4.9, 1.9, -1, -0.05, 0.001]], F)


def mixed_rays(rng, n, centers, radii, lo, size):
    """n rays with origins in the room lo .. lo + size, of the kinds of tests.test_receive_map_api.sweep_rays: axis-parallel, diagonal,
    with a zero component, starting inside a receiver, aimed to graze one, and plain; ray 0 is aimed at receiver 0's center."""
    lo, size = np.asarray(lo, F), np.asarray(size, F)
    K = centers.shape[0]
    o = lo + rng.uniform(0.02, 0.98, (n, 3)) * size
    d = rng.normal(size=(n, 3))
    kind = rng.integers(0, 7, n)
    ax = rng.integers(0, 3, n)
    for i in range(n):
        k = int(rng.integers(0, K))
        if kind[i] == 0:
            d[i] = 0.0
            d[i, ax[i]] = rng.choice([-1.0, 1.0])
        elif kind[i] == 1:
            d[i] = rng.choice([-1.0, 1.0], 3)
        elif kind[i] == 2:
            d[i, ax[i]] = 0.0
        elif kind[i] == 3:
            o[i] = centers[k] + rng.uniform(-0.5, 0.5, 3) * radii[k]
        elif kind[i] >= 4:
            d[i] = (centers[k] + rng.normal(size=3) * radii[k] * (0.7 if kind[i] == 4 else 0.3)) - o[i]
    d[0] = centers[0] - o[0]
    return np.ascontiguousarray(np.concatenate([o, d], axis=1))


def hash_name(name):
    return int.from_bytes(name.encode()[:8].ljust(8, b"\0"), "little") % (1 << 62) + len(name)


def edge_map_case(name, scene, rays, centers, radii, cell=0.0, expect=(), outside=False, B=1, bounces=2, mode="specular", directional=False,
                  partition="voxel", call="batch", n_bins=N_BINS, bin_len=BIN_LEN, frac_bits=30, rules=None, pack=1, state=False, shape="edge"):
    rng = np.random.default_rng(abs(hash_name(name)))
    P = mesh_of(scene)[0].shape[0]
    n = rays.shape[0]
    alpha = rng.uniform(0.05, 0.5, (P, B)) if B > 1 else None
    sigma = rng.uniform(0.0, 1.0, (P, B)) if mode != "specular" else None
    state_in = np.concatenate([rng.uniform(-0.5 * bin_len, 0.8 * n_bins * bin_len, (1, n)), rng.uniform(0.0, 2.0, (B, n))]) if state else None
    EXPECT[name] = tuple(expect)
    if outside:
        OUTSIDE.add(name)
    return Case(name, scene, PARTITIONS[partition], np.ascontiguousarray(rays, F), bounces, np.ascontiguousarray(centers, F), np.ascontiguousarray(radii, F),
                n_bins, bin_len, frac_bits, mode, directional, 1, pack, alpha, sigma, state_in, 4321, None, None, 1, call == "device", map_cell=cell,
                map_shape=shape, two_scenes=call == "sharded", **(rules or {}))


def exact_rays():
    return np.concatenate([axis_rays(), tie_rays(), pad_rays(), end_rays()])


def degenerate_layout(kind, K, size, rng):
    """(centers, radii, cell) of the degenerate grids: plane-<a> (coplanar centers, n_a == 1), line (two dims of 1), point (K coincident
    centers), fine (a caller's cell of 1/16 of the diameter: P about 8), all (a caller's cell that holds everything), big (one radius a
    hundred times the rest)."""
    size = np.asarray(size, F)
    c = rng.uniform(0.1, 0.9, (K, 3)) * size
    r = rng.uniform(0.15, 0.3, K)
    cell = 0.0
    if kind.startswith("plane-"):
        c[:, int(kind[-1])] = 0.4 * size[int(kind[-1])]
    elif kind == "line":
        c[:, 1], c[:, 2] = 0.5 * size[1], 0.3 * size[2]
    elif kind == "point":
        c[:] = np.array([0.31, 0.42, 0.37]) * size
    elif kind == "fine":
        r[:] = 0.32
        cell = 0.04
    elif kind == "all":
        cell = 64.0
    elif kind == "big":
        r[:] = 0.02
        r[K // 2] = 2.0
    return np.ascontiguousarray(c), r, cell


def special_rays(rng, n, centers, radii, size, huge=False):
    """n rays of which two in three are ordinary ones that detect (mixed_rays); the others hold the special values in origin and
    direction, the all-zero direction, and directions scaled by 2^600 (huge: all of the odd ones are)."""
    rays = mixed_rays(rng, n, centers, radii, np.zeros(3), size)
    sp = np.array(SPECIAL)
    for i in range(1, n, 3):
        if huge or i % 9 == 1:
            rays[i, 3:] *= 2.0 ** 600
            continue
        at = rng.random(6) < 0.4
        at[int(rng.integers(0, 6))] = True
        rays[i, at] = rng.choice(sp, int(at.sum()))
    rays[4, 3:] = 0.0
    rays[7] = [5.0, 3.0, 1.5, np.inf, np.inf, 1.0]                               # v * 0 = NaN on the major and on a minor axis: idx(NaN) = 0
    rays[10] = [5.0, 3.0, 1.5, 1.0, -np.inf, np.inf]
    return rays


def lost_case(rng):
    """Outside the domain with lost > 0: 64 receivers of 1 cm in a 2 m cube 2^50 m from the origin, where a double's step is 25 cm.  The
    linear test rounds o + d * s to that step and detects pairs whose cell the rule, exact in its cell units, does not visit; the map's
    own definition holds.  The rays are half-lines in the open soup near the origin."""
    T, K, n = 2.0 ** 50, 64, 257
    ce = T + rng.uniform(0.0, 2.0, (K, 3))
    ra = np.full(K, 0.01)
    k = rng.integers(0, K, n)
    o = T + rng.uniform(-1.0, 3.0, (n, 3))
    off = rng.normal(size=(n, 3))
    off /= np.linalg.norm(off, axis=1, keepdims=True)
    d = (ce[k] + off * ra[k, None] * rng.uniform(0.0, 1.3, (n, 1))) - o
    return edge_map_case("lost-far-grid", SOUP, np.concatenate([o, d], axis=1), ce, ra, B=3, directional=True, outside=True, expect=("lost", "half_line"))


def map_edge_cases():
    """The fixed cases at the visit rule's edges; EXPECT names, per case, the classes (MAP_TALLIES) it is there for, OUTSIDE the cases
    outside the header's domain.  What no case can hold: a DETECTION on a ray whose zero axis lies exactly on a padded face, or that
    only touches the padded grid (t0 == t1).  Such a ray's points are at least R = r_max + h / 8 from every center on that axis, and a
    detection needs less than r_k <= r_max: the faces' inclusiveness decides candidates there, never a histogram word.  The cases
    hold those rays (face_lo, face_hi, touch > 0, and candidates for them); beside them stand rays that detect."""
    EXPECT.clear()
    OUTSIDE.clear()
    size = np.array(mesh_of(EXACT_ROOM)[2])
    box = np.array(mesh_of(("shoebox",))[2])
    ec, er = exact_layout()
    rng = np.random.default_rng(20261019)
    fill = lambda rays, n: np.concatenate([rays, mixed_rays(rng, n - rays.shape[0], ec, er, np.zeros(3), size)])      # noqa: E731
    c = []
    # exact layouts
    c.append(edge_map_case("exact-axis", EXACT_ROOM, fill(axis_rays(), 63), ec, er, expect=("axis1", "axis2", "face_lo", "face_hi"), call="device"))
    c.append(edge_map_case("exact-ties", EXACT_ROOM, fill(tie_rays(), 64), ec, er, expect=("tie_major_same", "tie_major_opposite"), B=3, directional=True,
                           partition="octree"))
    touch_room = ("box", 1.25, 1.0, 1.0, 0.0, 0.0, -0.375)                       # its roof is the padded face z = 3.625
    touch = np.array([[4.25, 2.75, 6.0, 0, 0, -1], [4.25, 2.75, 6.0, 0, 0, -2], [6.5, 3.25, 8.0, 0, 0, -0.5], [3.0, 2.0, 5.0, 0.25, 0, -1]], F)
    c.append(edge_map_case("exact-touch", touch_room, fill(touch, 65), ec, er, expect=("touch", "enter", "leave"), B=8, mode="scatter", partition="kdtree"))
    c.append(edge_map_case("exact-pad-only", EXACT_ROOM, fill(pad_rays(), 255), ec, er, B=3, mode="scatter", directional=True,
                           expect=("pad_only",) + tuple(f"pad_only_{w}{a}" for w in ("major", "minor") for a in range(3)), call="sharded"))
    c.append(edge_map_case("exact-end-slab", EXACT_ROOM, fill(end_rays(), 256), ec, er, expect=("end_slab", "clamp_lo_slab", "clamp_hi_slab"), bounces=3))
    # a skipped slab: lo_x = 0, the ray starts at u_x = -2^-54 with v = (1, -0.5, 0) and leaves through the face u_y = -P at t1 = 0.375, so
    # a1 = 0.375 - 2^-54 and a1 + P rounds (a tie, to even) to 1.0: jhi = 1, but slab 1 begins at tA = 0.375 + 2^-54 > t1.  All exact.
    skip_room = ("box", 1.25, 1.0, 1.0, -1.0, 0.0, 0.0)
    skip = np.array([[-2.0 ** -54, 0.5625, 1.5, 1, -0.5, 0], [-2.0 ** -54, 0.5625, 1.5, 2, -1, 0], [-2.0 ** -54, 1.5, 0.5625, 4, 0, -2]], F)
    sc = ec - [1.0, 0.0, 0.0]
    rays = np.concatenate([skip, mixed_rays(rng, 60, sc, er, [-1.0, 0.0, 0.0], size)])
    c.append(edge_map_case("exact-skip", skip_room, rays, sc, er, expect=("slab_skipped",), B=3, directional=True))
    r2 = er.copy()
    r2[[k for k in range(100) if tuple(ec[k]) == (3.0, 2.0, 1.0)]] = 0.25
    r2[[k for k in range(100) if tuple(ec[k]) == (6.0, 2.0, 1.0)]] = np.nextafter(0.25, 1.0)
    c.append(edge_map_case("exact-r2", EXACT_ROOM, np.array([[0.5, 2.25, 1.0, 1, 0, 0]], F), ec, r2, expect=("axis2",)))
    # degenerate grids
    for j, (kind, K, n) in enumerate((("plane-0", 200, 257), ("plane-1", 257, 63), ("plane-2", 300, 64), ("line", 256, 65), ("point", 300, 255),
                                      ("fine", 40, 256), ("all", 255, 257), ("big", 300, 64))):
        ce, ra, cell = degenerate_layout(kind, K, box, rng)
        c.append(edge_map_case("grid-" + kind, ("shoebox",) if j % 2 else ("room",), mixed_rays(rng, n, ce, ra, np.zeros(3), box), ce, ra, cell,
                               B=(1, 3, 8)[j % 3], bounces=1 + j % 3, mode=("specular", "scatter")[j % 2], directional=j % 4 >= 2,
                               partition=("voxel", "octree", "kdtree")[j % 3], call=("batch", "device", "sharded")[j % 3], state=j % 2 == 0))
    c.append(edge_map_case("grid-K1", ("shoebox",), mixed_rays(rng, 1, ec[:1] * 0 + [3.0, 3.0, 2.0], er[:1], np.zeros(3), box), [[3.0, 3.0, 2.0]], [0.5],
                           bounces=3, call="device"))
    # the cell cap: 128 x 128 x 128 after the doubling of h, and 2^21 x 1 x 1; the rays start outside the grid and cross it
    K = 300
    corner = np.array([3.0, 1.5, 0.05])
    ce = corner + rng.uniform(0.0, 1.0, (K, 3)) * 3.9
    ce[0], ce[1] = corner, corner + 3.9
    ra = np.full(K, 0.0306 / 16)
    aim = rng.integers(0, K, 64)
    aim[:8] = np.arange(8) % 2                                                   # the grid's two corners: ranges that reach past its sides
    tg = ce[aim] + rng.normal(size=(64, 3)) * ra[0] * 0.4
    o = np.stack([np.where(np.arange(64) % 2 == 0, 0.3, 9.7), rng.uniform(0.3, 6.7, 64), rng.uniform(0.3, 3.7, 64)], axis=1)
    o[32:48] = np.stack([rng.uniform(3.0, 6.9, 16), np.where(np.arange(16) % 2 == 0, 0.3, 6.7), rng.uniform(0.3, 3.7, 16)], axis=1)
    o[48:56] = tg[48:56] * [1, 1, 0] + [0, 0, 0.02]                              # straight up from under the grid
    o[56:] = tg[56:] * [0, 1, 1] + [0.3, 0, 0]                                   # along x
    d = tg - o
    c.append(edge_map_case("cap-cube", ("shoebox",), np.concatenate([o, d], axis=1), ce, ra, B=3, directional=True, n_bins=96,
                           expect=("enter", "leave", "clamp_lo_range", "clamp_hi_range", "clamp_lo_slab", "clamp_hi_slab"), shape="cap"))
    ce = np.stack([1.0 + 8.0 * np.sort(rng.uniform(0.0, 1.0, K)), np.full(K, 3.5), np.full(K, 2.0)], axis=1)
    ce[0, 0], ce[-1, 0] = 1.0, 9.0
    ra = np.full(K, 0.01)
    o = np.stack([np.where(np.arange(64) % 2 == 0, 0.5, 9.5), 3.5 + rng.uniform(-0.005, 0.005, 64), 2.0 + rng.uniform(-0.005, 0.005, 64)], axis=1)
    d = np.stack([np.where(np.arange(64) % 2 == 0, 1.0, -1.0), np.zeros(64), np.zeros(64)], axis=1)
    d[32:, 1:] = rng.uniform(-1e-4, 1e-4, (32, 2))
    c.append(edge_map_case("cap-line", ("shoebox",), np.concatenate([o, d], axis=1), ce, ra, cell=8.0 / ((1 << 21) - 0.5), bounces=1,
                           expect=("enter", "leave", "clamp_lo_slab", "clamp_hi_slab", "end_slab"), shape="cap"))
    # scales and places
    for label, s in (("2^-20", 2.0 ** -20), ("2^30", 2.0 ** 30)):
        rays = fill(exact_rays(), 257)
        rays[:, :3] *= s
        c.append(edge_map_case("scale-" + label, ("box", 1.25 * s, s, s, 0.0, 0.0, 0.0), rays, ec * s, er * s, bin_len=BIN_LEN * s, B=3,
                               expect=("pad_only", "end_slab", "tie_major_opposite", "axis2"), call="device" if s < 1 else "batch"))
    T = 1047527.0                                                                # 0.999 x 2^20 cells of edge 1
    rays = fill(exact_rays(), 257)
    rays[:, :3] += T
    c.append(edge_map_case("far-origin", ("box", 1.25, 1.0, 1.0, T, T, T), rays, ec + T, er, B=3, mode="scatter", directional=True,
                           expect=("end_slab", "tie_major_opposite", "axis2", "enter"), call="sharded"))
    rays = fill(exact_rays(), 257)
    rays[:, 3:] *= 2.0 ** rng.integers(-30, 31, (257, 1))
    rays[17::64, 3:] *= TINY
    c.append(edge_map_case("dir-scaled", EXACT_ROOM, rays, ec, er, B=8, directional=True, expect=("pad_only", "end_slab", "tie_major_same"), bounces=3))
    # outside the domain: the histogram is still a function of the inputs
    c.append(edge_map_case("special-rays", EXACT_ROOM, special_rays(rng, 257, ec, er, size), ec, er, B=3, directional=True, outside=True,
                           expect=("clip_nan", "clamp_nan_slab", "clamp_nan_range", "touch"), call="device"))
    c.append(edge_map_case("special-scatter", ("room",), special_rays(rng, 257, ec, er, box), ec, er, B=8, mode="scatter", outside=True,
                           expect=("clip_nan",), partition="kdtree", call="sharded"))
    c.append(edge_map_case("huge-dir", EXACT_ROOM, special_rays(rng, 257, ec, er, size, huge=True), ec, er, B=1, outside=True, expect=("enter",)))
    c.append(lost_case(rng))
    # every form once more: whole blocks of 64 rays retire in an open soup; the rules
    ce, ra, cell = map_layout("cloud", 300, box, rng)
    for n, pack in ((4095, 0), (4096, 1), (4159, 0), (4159, 1)):
        c.append(edge_map_case(f"soup-{n}-pack{pack}", SOUP, scenes.random_rays(n, box, seed=n + pack), ce, ra, cell, B=(1, 3)[pack], bounces=3,
                               mode=("scatter", "specular")[pack], directional=n == 4159, pack=pack, expect=("half_line",),
                               partition=("octree", "voxel")[pack], call="device" if n == 4096 else "batch"))
    c.append(edge_map_case("edge-time-limit", EXACT_ROOM, fill(exact_rays(), 4097), ec, er, B=3, bounces=4, mode="scatter", n_bins=24,
                           rules=dict(time_limit=True), expect=("pad_only",)))
    c.append(edge_map_case("edge-floor-roulette", EXACT_ROOM, fill(exact_rays(), 4097), ec, er, B=3, bounces=4, directional=True,
                           rules=dict(floor_bits=2, roulette=True), expect=("pad_only",), call="sharded"))
    # K > 256 on the exact pad: radii 0.25 on the half-integers, h = 0.5, P = 0.625 (also the case of the _reduced calls)
    hc = np.stack(np.meshgrid(np.arange(0.5, 12.25, 0.5), np.arange(0.5, 6.75, 0.5), np.arange(1.0, 2.25, 0.5), indexing="ij"), axis=-1).reshape(-1, 3)
    hr = np.full(hc.shape[0], 0.25)
    rays = np.concatenate([exact_rays(), mixed_rays(rng, 257 - exact_rays().shape[0], hc, hr, np.zeros(3), size)])
    c.append(edge_map_case("exact-half-K936", EXACT_ROOM, rays, hc, hr, B=3, bounces=3, n_bins=64, frac_bits=40,
                           expect=("pad_only", "end_slab", "tie_major_opposite", "axis2")))
    names = [x.name for x in c]
    assert len(set(names)) == len(names)
    return c


# ---- the seeded sweep (tests/test_gpu_receive_map_sweep.py, tools/fuzz_receive.py with MAP=1)
SWEEP_LAYOUTS = ("plane", "cloud", "coincident", "big", "onecell", "cell", "plane-0", "plane-1", "plane-2", "line", "point", "fine", "all")
PAIRS_MAX = 1 << 24                      # n x K: the reference's masks


def map_sweep_case(seed):
    """One map case from the seed; nothing is redrawn.  Drawn: the layout (map_layout's six and degenerate_layout's), K = 1 .. 4096 (three
    seeds in ten above 256; one in twenty 16 384 .. 65 536 with few bins and rays), the cell (0, or 1/16 .. 64 of the diameter), the
    room (the shoebox scaled by 2^-10 .. 2^10 per axis and shifted by up to 2^19 cells, or unscaled: shoebox, partition room, soup), the
    rays (mixed_rays; one seed in five sprinkled with SPECIAL), 1 .. 4 casts, the four forms, the three partitions, B = 1 .. 8,
    frac_bits 0 .. 62, bounce_pack, the rules in a quarter of the seeds, a starting state or none, one scene or two.  Receiver 0 lies
    on ray 0's path, half way to its first hit, with L = 0 and a bin length that bins it."""
    rng = np.random.default_rng(0x3A90000 + int(seed))
    r = rng.random()
    if seed % 20 == 7:
        K = int(rng.integers(16384, 65537))
    elif r < 0.32:
        K = int(np.exp(rng.uniform(np.log(257.0), np.log(4097.0))))
    else:
        K = max(1, min(256, int(np.exp(rng.uniform(0.0, np.log(257.0))))))
    big = K > 4096
    n = int(rng.integers(1, 65)) if big else min(PAIRS_MAX // K, int(rng.choice([1, 63, 64, 65, 255, 256, 257, int(rng.integers(1, 1500))])))
    which = int(rng.integers(0, 6))
    base = np.array(mesh_of(("shoebox",))[2])
    if which <= 2:
        s = 2.0 ** rng.integers(-10, 11, 3).astype(F)
        scene, scale = None, s
    else:
        scene, scale = (("shoebox",), ("room",), SOUP)[which - 3], np.ones(3)
    size = base * scale
    layout = SWEEP_LAYOUTS[int(rng.integers(0, len(SWEEP_LAYOUTS)))]
    if big and layout in ("point", "coincident"):
        layout = "cloud"                 # tens of thousands of coincident receivers are K deposits per ray: 40 s of reference for one seed
    if layout in ("plane", "cloud", "coincident", "big", "onecell", "cell"):
        centers, radii, cell = map_layout(layout, K, base, rng)
    else:
        centers, radii, cell = degenerate_layout(layout, K, base, rng)
    if big:
        radii = radii * 0.2
    centers = centers * scale
    radii = radii * float(scale.min())
    cell = cell * float(scale.min())
    if cell == 0.0 and rng.random() < 0.4:
        cell = 2.0 * float(radii.max()) * float(2.0 ** rng.integers(-4, 7))
    rays = mixed_rays(rng, n, centers, radii, np.zeros(3), size)
    rays[1:, 3:] *= 2.0 ** rng.integers(-30, 31, (n - 1, 1)) if rng.random() < 0.3 else 1.0      # ray 0 ends short of the walls at s = 1
    shift = np.zeros(3)
    if scene is None:
        h = build_grid(centers, radii, cell).h
        shift = np.rint(rng.uniform(-1.0, 1.0, 3) * 2.0 ** rng.integers(0, 20)) * h * (rng.random() < 0.7)
        scene = ("box",) + tuple(float(x) for x in scale) + tuple(float(x) for x in shift)
        centers, rays = centers + shift, rays.copy()
        rays[:, :3] += shift
    # receiver 0 on ray 0's path: half way to its first hit, or a unit of its parameter along a ray that leaves
    ev = po.brute(po.Topology(*mesh_of(scene)[:2]), rays[:1])
    ev = ev[0] if isinstance(ev, tuple) else ev
    t_rcv = float(ev["t"][0]) * 0.5 if int(ev["hit"][0]) == 1 else 1.0
    centers[0] = rays[0, :3] + rays[0, 3:] * t_rcv
    if seed % 5 == 3:
        at = rng.random((n, 6)) < 0.08
        at[0] = False
        rays[at] = rng.choice(np.array(SPECIAL), int(at.sum()))
    P = mesh_of(scene)[0].shape[0]
    B = int(rng.integers(1, 9))
    mode = ("specular", "scatter")[int(rng.integers(0, 2))]
    bounces = int(rng.integers(1, 5))
    n_bins = int(rng.integers(1, 9)) if big else int(np.exp(rng.uniform(0.0, np.log(min(2001.0, (1 << 22) / (K * B * 4))))))
    n_bins = max(1, min(n_bins, (1 << 22) // (K * B * 4)))
    bin_len = 8.0 * t_rcv / n_bins * float(np.exp(rng.uniform(np.log(0.5), np.log(4.0))))      # x of that detection: n_bins / (4 .. 32)
    alpha = rng.uniform(0.0, 0.7, (P, B)) if B > 1 or rng.random() < 0.5 else None
    sigma = rng.uniform(0.0, 1.0, (P, B)) if mode != "specular" else None
    state_in = None
    if rng.random() < 0.5:
        state_in = np.concatenate([rng.uniform(0.0, 0.5 * n_bins * bin_len, (1, n)), rng.uniform(0.0, 2.0, (B, n))])
        state_in[0, 0] = 0.0
    kind = ("voxel", "octree", "kdtree")[int(rng.integers(0, 3))]
    if kind == "octree" and scene[0] == "box":
        kind = ("voxel", "kdtree")[seed % 2]          # the octree pads its nodes by an absolute 0.1 m: not for a room of millimetres
    rules = {}
    if seed % 4 == 1:
        rules = dict(time_limit=bool(rng.integers(0, 2)), floor_bits=int(rng.integers(0, 4)), roulette=bool(rng.integers(0, 2)))
        rules["time_limit"] = rules["time_limit"] or rules["floor_bits"] == 0
    case = Case(f"map-sweep-{seed}", scene, PARTITIONS[kind], np.ascontiguousarray(rays), bounces, np.ascontiguousarray(centers), np.ascontiguousarray(radii),
                n_bins, bin_len, int(rng.integers(0, 63)), mode, bool(rng.integers(0, 2)), 1, int(rng.integers(0, 2)), alpha, sigma, state_in,
                int(rng.integers(-(1 << 63), (1 << 63) - 1, endpoint=True)), None, None, 1, False, map_cell=cell, map_shape=layout,
                two_scenes=bool(rng.random() < 0.2), **rules)
    assert case.n * case.K <= PAIRS_MAX and case.words <= 1 << 22
    return case
