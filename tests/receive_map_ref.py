"""numpy restatement of receiver maps (include/hare_hip.h, "receivers", "Receiver maps"), operation for operation in FP64: the grid the
setter builds (build_grid: cells, CSR) and the visit rule as a candidate mask per ray and cast (candidates).  The loop is
tests.receive_ref.receive_loop with visit=functools.partial(candidates, grid): its receiver step then runs, per receiver, on the rays
that hold the receiver as a candidate (a map refuses the rain).

Below it: the cases that the CPU tests (tests/test_receive_map_api.py) and the device tests (tests/test_gpu_receive_map.py) share --
plain tests.receive_cases.Case records with map_cell set, run by tests.receive_cases.reference like every other case."""
import dataclasses

import numpy as np

import hare_amd.scenes as scenes
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


def candidates(g, o, d, t_end):
    """The visit rule: bool [m, K], True where the cell of receiver k is visited by ray i (o, d [m, 3]; t_end [m], +inf for a miss)."""
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
        ok &= (t0 <= t1) & (t1 < np.inf)
        major = np.zeros(m_rays, np.int64)
        vm = v[:, 0].copy()
        for a in (1, 2):
            big = np.abs(v[:, a]) > np.abs(vm)
            major = np.where(big, a, major)
            vm = np.where(big, v[:, a], vm)
        ok &= ~(vm == 0)
        um = u[np.arange(m_rays), major]
        a0, a1 = um + vm * t0, um + vm * t1
        amin, amax = np.where(a0 < a1, a0, a1), np.where(a0 < a1, a1, a0)
        for mm in range(3):
            rows = np.nonzero(ok & (major == mm))[0]
            if rows.size == 0:
                continue
            nm = int(g.dims[mm])
            jlo, jhi = _idx(np.floor(amin[rows] - P), nm), _idx(np.floor(amax[rows] + P), nm)
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
                for a in others:
                    p0, p1 = u[rr, a] + v[rr, a] * ts, u[rr, a] + v[rr, a] * te
                    pmin, pmax = np.where(p0 < p1, p0, p1), np.where(p0 < p1, p1, p0)
                    lo_a, hi_a = _idx(np.floor(pmin - P), int(g.dims[a])), _idx(np.floor(pmax + P), int(g.dims[a]))
                    ca = g.cell_of[ks, a][None, :]
                    inside &= (lo_a[:, None] <= ca) & (ca <= hi_a[:, None])
                cand[np.ix_(rr, ks)] = inside
    return cand


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
