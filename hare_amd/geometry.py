"""Host-side mirror of the reference's interface for the ray-cast path, over the C-ABI.

Same names, argument meaning and error behaviour as Hare.Geometry's
  Ray / X_Event            Hare_Geometry_Primitives.cs:393-481
  Topology (the members a partition reads)   Hare_Geometry_Topology.cs:418-424, :482, :539, :50/:58
  Spatial_Partition        Spatial_Partition.cs:27-35
  Voxel_Grid / Octree / KDTree constructors  Voxel_Grid.cs:48,128  "Octree - alt.cs":45  KDTree.cs:51
so the parity tests read like calls into the reference.  Every Shoot runs the HIP kernels through
libhare_hip.so; there is no Python or CPU implementation of the path in this package.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import capi
from .capi import KIND_KDTREE, KIND_OCTREE, KIND_VOXEL, RAY_DTYPE, XEVENT_DTYPE, check, lib, ptr


class Ray:
    """Hare.Geometry.Ray (Hare_Geometry_Primitives.cs:393-429)."""

    __slots__ = ("x", "y", "z", "dx", "dy", "dz", "ThreadID", "Ray_ID", "poly_origin1", "poly_origin2")

    def __init__(self, x, y, z, dx, dy, dz, ThreadID_IN: int = 0, ID: int = 0):
        self.x, self.y, self.z = float(x), float(y), float(z)
        self.dx, self.dy, self.dz = float(dx), float(dy), float(dz)
        self.ThreadID, self.Ray_ID = int(ThreadID_IN), int(ID)
        self.poly_origin1 = self.poly_origin2 = 0

    def Reverse(self):
        self.dx *= -1
        self.dy *= -1
        self.dz *= -1


class X_Event:
    """Hare.Geometry.X_Event (Hare_Geometry_Primitives.cs:435-481)."""

    __slots__ = ("u", "v", "t", "Hit", "X_Point", "Poly_id")

    def __init__(self, P=None, u_in=0.0, v_in=0.0, t_in=0.0, Poly_index=-1):
        if P is None:           # X_Event(): :454-462
            self.u = self.v = self.t = 0.0
            self.Hit = False
            self.X_Point = None
            self.Poly_id = -1
        else:                   # X_Event(Point, u, v, t, Poly_index): :472-480
            self.u, self.v, self.t = float(u_in), float(v_in), float(t_in)
            self.Hit = True
            self.X_Point = tuple(float(c) for c in P)
            self.Poly_id = int(Poly_index)

    @staticmethod
    def from_record(r) -> "X_Event":
        if r["hit"]:
            return X_Event((r["x"], r["y"], r["z"]), r["u"], r["v"], r["t"], r["poly_id"])
        return X_Event()


class Topology:
    """The part of Hare.Geometry.Topology a Spatial_Partition reads: polygons with their corner
    coordinates, unit normals and the Min/Max box (after Finish_Topology).  Normals and bounds are
    computed by the library's restatements of the Polygon ctor / Finish_Topology."""

    def __init__(self, verts, nverts=None, normals=None, Min=None, Max=None):
        v = np.ascontiguousarray(verts, np.float64)
        if v.ndim == 3 and v.shape[1] == 3:      # [P,3,3] triangles
            w = np.zeros((v.shape[0], 4, 3), np.float64)
            w[:, :3] = v
            v = w
        self.verts = np.ascontiguousarray(v.reshape(-1, 4, 3))
        P = self.verts.shape[0]
        self.nverts = np.full(P, 3, np.int32) if nverts is None else np.ascontiguousarray(nverts, np.int32)
        if self.nverts.shape != (P,):
            raise ValueError("nverts must have one entry per polygon")
        if normals is None:
            normals = np.zeros((P, 3), np.float64)
            check(lib.hare_polygon_normals(ptr(self.verts), ptr(self.nverts), P, ptr(normals)))
        self.normals = np.ascontiguousarray(normals, np.float64)
        if Min is None or Max is None:
            Min = np.zeros(3)
            Max = np.zeros(3)
            check(lib.hare_topology_bounds(ptr(self.verts), ptr(self.nverts), P, ptr(Min), ptr(Max)))
        self.Min = np.ascontiguousarray(Min, np.float64)
        self.Max = np.ascontiguousarray(Max, np.float64)

    @classmethod
    def from_polygons(cls, T, nverts=None):
        """Topology(Point[][] T) (Hare_Geometry_Topology.cs:120-142) followed by Finish_Topology(): the raw
        corners go through the reference's ingest (Math.Round(x, 15), corners in the same 1 mm Hash2 cell
        merged onto the first one) before normals and bounds are taken.  `T` is [P,3,3], [P,4,3] or a
        sequence of 3- or 4-corner polygons; `nverts` overrides the corner count per polygon.
        The result also carries Vertices_List (`.vertices`) and the per-corner vertex index (`.corner_vertex`)."""
        if not isinstance(T, np.ndarray):
            polys = [np.asarray(p, np.float64).reshape(-1, 3) for p in T]
            soup = np.zeros((len(polys), 4, 3), np.float64)
            nverts = np.zeros(len(polys), np.int32)
            for i, p in enumerate(polys):
                if p.shape[0] not in (3, 4):
                    raise NotImplementedError("Hare Does not yet support polygons of more than 4 sides.")
                soup[i, :p.shape[0]] = p
                nverts[i] = p.shape[0]
        else:
            v = np.ascontiguousarray(T, np.float64)
            soup = np.zeros((v.shape[0], 4, 3), np.float64)
            soup[:, :v.shape[1]] = v
            if nverts is None:
                nverts = np.full(v.shape[0], v.shape[1], np.int32)
        nverts = np.ascontiguousarray(nverts, np.int32)
        P = soup.shape[0]
        verts = np.zeros((P, 4, 3), np.float64)
        corner_vertex = np.full((P, 4), -1, np.int32)
        vertices = np.zeros((max(int(nverts.sum()), 1), 3), np.float64)
        nv = C.c_int32(0)
        rc = lib.hare_topology_ingest(ptr(soup), ptr(nverts), P, ptr(verts), ptr(corner_vertex), ptr(vertices), C.addressof(nv))
        if rc == capi.HARE_E_UNSUPPORTED:
            raise NotImplementedError(capi.last_error())
        check(rc)
        top = cls(verts, nverts)
        top.vertices = vertices[:nv.value].copy()
        top.corner_vertex = corner_vertex
        return top

    @property
    def Polygon_Count(self) -> int:
        return int(self.verts.shape[0])

    def Normal(self, Poly_ID: int):
        return tuple(self.normals[Poly_ID])

    def __getitem__(self, key):
        poly, corner = key
        return tuple(self.verts[poly, corner])

    def Polygon_Vertices(self, Poly_ID: int):
        return [tuple(self.verts[Poly_ID, c]) for c in range(int(self.nverts[Poly_ID]))]

    def _desc(self) -> capi.TopologyDesc:
        d = capi.TopologyDesc()
        d.P = self.Polygon_Count
        d.verts = ptr(self.verts)
        d.nverts = ptr(self.nverts)
        d.normals = ptr(self.normals)
        for a in range(3):
            d.min[a] = self.Min[a]
            d.max[a] = self.Max[a]
        return d


def _result_array(out, shape, dtype):
    """The result array of a host-buffer call: a fresh one, or the caller's `out` -- checked, never converted: the library writes
    straight into it.  Reusing one array across calls saves its first-touch page faults (56 B per ray: 1M rays 13.6 ms -> 1.9 ms
    per hare_shoot_batch_sharded call on an MI355X host, round 6)."""
    if out is None:
        return np.zeros(shape, dtype)
    shape = (shape,) if isinstance(shape, (int, np.integer)) else tuple(shape)
    if not (isinstance(out, np.ndarray) and out.dtype == dtype and out.shape == shape and out.flags.c_contiguous and out.flags.writeable):
        raise ValueError("out must be a writeable C-contiguous array of %d-byte result records with shape %s" % (np.dtype(dtype).itemsize, shape))
    return out


def decay_levels(dB_list):
    """The levels of a reduction (include/hare_hip.h, "receivers", "Reduction") from decibels <= 0: uint32 fractions in units of 2^-32,
    min(2^32 - 1, floor(10^(dB / 10) * 2^32)) -- -5 dB is floor(10^-0.5 * 2^32).  A host convenience that produces data: whatever uint32
    values the caller passes are the definition's f_l."""
    dB = np.asarray(dB_list, np.float64).reshape(-1)
    if not (np.isfinite(dB).all() and (dB <= 0).all()):
        raise ValueError("levels are finite decibels <= 0")
    return np.minimum(np.floor(10.0 ** (dB / 10.0) * 4294967296.0), 4294967295.0).astype(np.uint32)


def air_weights(m, bin_len: float, n_bins: int):
    """The weights of a reduction for air absorption: m [B], the energy attenuation per unit of path length in each band; returns uint32
    [n_bins, B] in units of 2^-32, min(2^32 - 1, floor(exp(-m_b * (i + 0.5) * bin_len) * 2^32)): the attenuation at the middle of bin i.  A
    host convenience that produces data, like decay_levels."""
    m = np.asarray(m, np.float64).reshape(-1)
    if not (np.isfinite(m).all() and (m >= 0).all()):
        raise ValueError("attenuation coefficients are finite and >= 0")
    mid = (np.arange(int(n_bins), dtype=np.float64) + 0.5) * float(bin_len)
    return np.minimum(np.floor(np.exp(-m[None, :] * mid[:, None]) * 4294967296.0), 4294967295.0).astype(np.uint32)


def band_taps(fs: float, edges, T: int):
    """Band filters for hist_render: float64 [B, T] with B = len(edges) + 1, T odd.  Lowpass l is the Hamming-windowed sinc of cut-off
    edges[l] (Hz, ascending, below fs / 2), scaled to unit gain at 0 Hz; band 0 is lowpass 0, band b is lowpass b minus lowpass b - 1, and
    the top band is the unit impulse at (T - 1) / 2 minus the last lowpass: the bands telescope to a pure delay of (T - 1) / 2 samples.  A
    host convenience that produces data: whatever taps the caller passes are the definition's."""
    T = int(T)
    edges = np.asarray(edges, np.float64).reshape(-1)
    if T < 1 or T % 2 == 0:
        raise ValueError("T must be odd and >= 1")
    if not (np.isfinite(fs) and fs > 0 and np.isfinite(edges).all() and (edges > 0).all() and (edges < fs / 2).all() and (np.diff(edges) > 0).all()):
        raise ValueError("edges are ascending frequencies in (0, fs / 2)")
    n = np.arange(T, dtype=np.float64) - (T - 1) / 2
    window = np.hamming(T) if T > 1 else np.ones(1)
    low = [np.sinc(2.0 * f / fs * n) * window for f in edges]
    low = [h / h.sum() for h in low]
    delta = np.zeros(T)
    delta[(T - 1) // 2] = 1.0
    steps = [np.zeros(T)] + low + [delta]
    return np.ascontiguousarray([steps[b + 1] - steps[b] for b in range(len(edges) + 1)])


def unit_energy_taps(taps):
    """taps float64 [B, T] with every band's row scaled to unit energy (the sum of its squares 1): an impulse of hist_impulses then puts
    the histogram's energy e into its band, as hist_render's noise does over a bin.  A row of zeros stays as it is.  A host convenience
    that produces data: whatever taps the caller passes are the definition's."""
    taps = np.array(taps, np.float64, ndmin=2)
    if taps.ndim != 2 or not np.isfinite(taps).all():
        raise ValueError("taps must be finite float64 [B, T]")
    norm = np.sqrt((taps * taps).sum(axis=1, keepdims=True))
    return np.ascontiguousarray(taps / np.where(norm > 0, norm, 1.0))


def sums_to_float(sums):
    """The sums of a reduction [..., 4] (S0 lo, S0 hi, S1 lo, S1 hi; uint64) as float64 (S0, S1): rounded, for the ratios a caller forms."""
    s = np.asarray(sums).astype(np.float64)
    return s[..., 0] + s[..., 1] * 2.0 ** 64, s[..., 2] + s[..., 3] * 2.0 ** 64


def proj_to_int(proj):
    """The sums of a projection [..., 2] (lo, hi; uint64) as an object array [...] of Python integers: the 128-bit two's complement read
    exactly."""
    p = np.asarray(proj, np.uint64)
    lo, hi = p[..., 0].astype(object), p[..., 1].astype(object)
    v = lo + hi * (1 << 64)
    return v - (hi >> 63) * (1 << 128)


def _project_coef(coef, n_bins: int):
    """coef of a projection as a C-contiguous int32 [J, n_bins]; values outside int32 are an error, never wrapped."""
    c = np.asarray(coef)
    if c.ndim != 2 or c.shape[1] != n_bins or c.shape[0] < 1:
        raise ValueError("coef must be int32 [J, n_bins] = [J, %d], J >= 1" % n_bins)
    if c.dtype != np.int32:
        if c.dtype.kind not in "iu" or (c.size and (int(c.max()) > 2 ** 31 - 1 or int(c.min()) < -2 ** 31)):
            raise ValueError("coef must hold integers within int32")
    return np.ascontiguousarray(c, np.int32)


def _reduce_spec(reduce, n_bins: int, B: int):
    """reduce = dict(windows=[(lo, hi), ...] or None, levels=uint32 array or None, weight=uint32 [n_bins, B] or None), checked for shape
    only (the library checks the values): (weight, n_win, win, n_lev, levels), arrays or None."""
    unknown = set(reduce) - {"windows", "levels", "weight"}
    if unknown:
        raise ValueError("reduce: unknown keys %s" % sorted(unknown))
    win = reduce.get("windows")
    win = None if win is None else np.ascontiguousarray(win, np.int32).reshape(-1, 2)
    lev = reduce.get("levels")
    lev = None if lev is None else np.ascontiguousarray(lev, np.uint32).reshape(-1)
    w = reduce.get("weight")
    if w is not None:
        w = np.ascontiguousarray(w, np.uint32)
        if w.shape != (int(n_bins), int(B)):
            raise ValueError("weight must be uint32 [n_bins, B] = [%d, %d]" % (n_bins, B))
    return w, 0 if win is None else win.shape[0], win, 0 if lev is None else lev.shape[0], lev


def _hist_shape(hist):
    """A histogram as the receive calls return it, for hist_reduce, hist_project and hist_render: (hist, K, n_bins, B, channels), hist
    contiguous uint64 [K, n_bins, B] (channels = 1) or [K, n_bins, B, C] (channels = C = 4, 9 or 16)."""
    hist = np.ascontiguousarray(hist, np.uint64)
    if hist.ndim not in (3, 4) or (hist.ndim == 4 and hist.shape[3] not in (4, 9, 16)):
        raise ValueError("hist must be uint64 [K, n_bins, B] or [K, n_bins, B, C], C = 4, 9 or 16")
    return (hist,) + hist.shape[:3] + (hist.shape[3] if hist.ndim == 4 else 1,)


class Spatial_Partition:
    """Hare.Geometry.Spatial_Partition (Spatial_Partition.cs:27-35) over a native scene."""

    _kind = -1

    #: Opt-in (default off): reproduce the reference's `Ray_ID == 0` rule.  Voxel_Grid.Shoot and KDTree.Shoot skip a polygon whose
    #: mailbox entry equals R.Ray_ID (Voxel_Grid.cs:687-689, KDTree.cs:224-229) and the mailbox starts out all zero, so a ray with
    #: Ray_ID == 0 finds every polygon "already tested" and the reference returns X_Event() -- after moving an outside origin as for
    #: any ray.  The GPU classes keep no mailbox and return the hit; with this switch on, Shoot(R) with
    #: R.Ray_ID == 0 and Shoot_batch(..., ray_ids=) entries equal to 0 return the miss record on Voxel_Grid and KDTree.  (The
    #: reference's rule is stateful -- a polygon some OTHER ray of the same ThreadID tested since is no longer skipped; the switch
    #: reproduces the fresh-mailbox case, which is the one a caller that forgot to assign ids meets.)  Octree has no mailbox.
    mailbox_ray_id0 = False

    def __init__(self, Model_in: Sequence[Topology], device: int = 0):
        self.Model = list(Model_in)
        self.Char_Step = 0.0
        descs = (capi.TopologyDesc * len(self.Model))(*[t._desc() for t in self.Model])
        h = C.c_void_p()
        check(lib.hare_scene_create(descs, len(self.Model), int(device), C.byref(h)))
        self._h = h
        self.device = int(device)

    def set_option(self, name: str, value: int):
        """Diagnostics / A-B switch of this scene (hare_scene_set_option): e.g. ("voxel_kernel", 2) forces the pool kernel."""
        check(lib.hare_scene_set_option(self._h, name.encode(), int(value)))
        return self

    def get_option(self, name: str) -> int:
        """hare_scene_get_option: an option read back, or "voxel_tight_bytes" / "octree_scratch_bytes" (device memory of the accelerators)."""
        v = C.c_int64()
        check(lib.hare_scene_get_option(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def close(self):
        if getattr(self, "_h", None):
            lib.hare_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # bool Shoot(Ray R, int top_index, out X_Event Ret_event[, int poly_origin1, int poly_origin2 = -1])
    def Shoot(self, R: Ray, top_index: int, poly_origin1: int = -1, poly_origin2: int = -1):
        """One ray, like the reference call site: runs on the calling host thread (hare_shoot_one -- a GPU round trip
        per ray would be ~100x slower than the reference), bit-identical to the batch kernels.  Returns (Hit, X_Event)."""
        ray = np.array([R.x, R.y, R.z, R.dx, R.dy, R.dz], np.float64)
        ev = np.zeros(1, XEVENT_DTYPE)
        check(lib.hare_shoot_one(self._h, self._kind, int(top_index), ptr(ray), int(poly_origin1), int(poly_origin2), ptr(ev)))
        R.x, R.y, R.z = (float(c) for c in ray[:3])       # the reference moves R when it starts outside (F11)
        if self.mailbox_ray_id0 and self._kind != KIND_OCTREE and int(getattr(R, "Ray_ID", 1)) == 0:
            return False, X_Event()                      # Voxel_Grid.cs:687-689 / KDTree.cs:224-229 on a fresh mailbox
        e = X_Event.from_record(ev[0])
        return e.Hit, e

    def Shoot_one(self, ray6, top_index: int = 0, poly_origin1: int = -1, poly_origin2: int = -1):
        """hare_shoot_one on a raw [x,y,z,dx,dy,dz] array (updated in place like the reference moves R); returns the record."""
        ev = np.zeros(1, XEVENT_DTYPE)
        check(lib.hare_shoot_one(self._h, self._kind, int(top_index), ptr(ray6), int(poly_origin1), int(poly_origin2), ptr(ev)))
        return ev[0]

    def Occluded_batch(self, rays, t_max=None, top_index: int = 0, poly_origin1=None, poly_origin2=None, events: bool = True,
                       simple_kernel: bool = False):
        """Harness-defined occlusion predicate: closest hit exists and t < t_max (t_max None: any hit).
        Returns (occluded int32[n], events) -- or, with events=False, (occluded, counters): flags only, from the kernels that
        end a ray's traversal as soon as its flag is decided (hits = number of occluded rays)."""
        rays = np.array(rays, np.float64, order="C").reshape(-1, 6)
        n = rays.shape[0]
        occ = np.zeros(n, np.int32)
        out = np.zeros(n, XEVENT_DTYPE) if events else None
        tm = None if t_max is None else np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, np.float64), (n,)))
        e1 = None if poly_origin1 is None else np.ascontiguousarray(poly_origin1, np.int32)
        e2 = None if poly_origin2 is None else np.ascontiguousarray(poly_origin2, np.int32)
        ctr = capi.Counters()
        check(lib.hare_occluded_batch(self._h, self._kind, int(top_index), n, ptr(rays), ptr(e1), ptr(e2), ptr(tm),
                                      capi.SHOOT_SIMPLE_KERNEL if simple_kernel else 0, ptr(occ), ptr(out), C.addressof(ctr)))
        return (occ, out) if events else (occ, ctr.as_dict())

    def occluded_device(self, n: int, d_rays: int, d_events: int, d_occluded: int, d_tmax: int = 0, top_index: int = 0,
                        d_excl1: int = 0, d_excl2: int = 0, d_counters: int = 0, stream: int = 0, flags: int = 0):
        check(lib.hare_occluded_device(self._h, self._kind, int(top_index), int(n), d_rays or None, d_excl1 or None,
                                       d_excl2 or None, d_tmax or None, int(flags), d_events or None, d_occluded or None,
                                       d_counters or None, stream or None))

    def Shoot_batch(self, rays, top_index: int = 0, poly_origin1=None, poly_origin2=None,
                    writeback_origin: bool = False, count_work: bool = False, simple_kernel: bool = False, slim: bool = False,
                    ray_ids=None, out=None):
        """n rays [n,6] through the HIP kernel (host buffers).  Returns (events, counters dict).
        With writeback_origin the rays array is updated in place like the reference mutates R.
        slim=True: the events come back as slim records (capi.SLIM_DTYPE for Voxel_Grid, SLIM_UV_DTYPE for the trees; 16 / 32
        bytes over the host link instead of 56); expand_events(rays, records) rebuilds the X_Events bit for bit.
        ray_ids (optional, one Ray_ID per ray) only matters with `mailbox_ray_id0` on: entries equal to 0 come back as miss records.
        out (optional): the caller's result array [n] of the dtype the call returns, written in place and returned (a caller that
        keeps it across calls does not pay a fresh array's page faults)."""
        if writeback_origin and not (isinstance(rays, np.ndarray) and rays.dtype == np.float64 and rays.flags.c_contiguous):
            rays = np.array(rays, np.float64, order="C")              # nothing of the caller's to write back into
        else:
            rays = np.ascontiguousarray(rays, np.float64)             # without the flag the library only reads them: no copy of 48 B per ray
        rays = rays.reshape(-1, 6)
        n = rays.shape[0]
        out = _result_array(out, n, self._slim_dtype() if slim else XEVENT_DTYPE)
        e1 = None if poly_origin1 is None else np.ascontiguousarray(poly_origin1, np.int32)
        e2 = None if poly_origin2 is None else np.ascontiguousarray(poly_origin2, np.int32)
        for e in (e1, e2):
            if e is not None and e.shape != (n,):
                raise ValueError("poly_origin arrays must have one entry per ray")
        flags = ((capi.SHOOT_WRITEBACK_ORIGIN if writeback_origin else 0) | (capi.SHOOT_COUNT_WORK if count_work else 0)
                 | (capi.SHOOT_SIMPLE_KERNEL if simple_kernel else 0) | (capi.SHOOT_SLIM_EVENTS if slim else 0))
        ctr = capi.Counters()
        check(lib.hare_shoot_batch(self._h, self._kind, int(top_index), n, ptr(rays), ptr(e1), ptr(e2), flags,
                                   ptr(out), C.addressof(ctr)))
        ctr = ctr.as_dict()
        if self.mailbox_ray_id0 and ray_ids is not None and self._kind != KIND_OCTREE:
            zero = np.asarray(ray_ids).reshape(-1) == 0
            if zero.shape != (n,):
                raise ValueError("ray_ids must have one entry per ray")
            if zero.any():
                ctr["hits"] -= int(np.count_nonzero(out["hit"][zero]))
                miss = np.zeros(1, out.dtype)
                miss["poly_id"] = -1
                out[zero] = miss[0]
        return out, ctr

    def _slim_dtype(self):
        return capi.SLIM_DTYPE if self._kind == KIND_VOXEL else capi.SLIM_UV_DTYPE

    def expand_events(self, rays, slim_records):
        """hare_expand_events: slim records (of a Shoot_batch(..., slim=True) on these rays, as they were passed in) -> X_Events."""
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        rec = np.ascontiguousarray(slim_records, self._slim_dtype())
        out = np.zeros(len(rec), XEVENT_DTYPE)
        check(lib.hare_expand_events(self._h, self._kind, len(rec), ptr(rays), ptr(rec), ptr(out)))
        return out

    @staticmethod
    def Shoot_batch_sharded(partitions, rays, top_index: int = 0, poly_origin1=None, poly_origin2=None,
                            writeback_origin: bool = False, slim: bool = False, out=None):
        """One batch over several devices from one process: `partitions` are equal partitions built on different
        devices (e.g. [Voxel_Grid(model, 64, device=k) for k in range(G)]); rays are split into contiguous shards in
        that order (hare_shoot_batch_sharded).  Returns (events, summed counters), byte-identical to Shoot_batch.
        out (optional): the caller's result array, as in Shoot_batch."""
        parts = list(partitions)
        if not parts or any(p._kind != parts[0]._kind for p in parts):
            raise ValueError("need one or more partitions of the same kind")
        if writeback_origin and not (isinstance(rays, np.ndarray) and rays.dtype == np.float64 and rays.flags.c_contiguous):
            rays = np.array(rays, np.float64, order="C")              # nothing of the caller's to write back into
        else:
            rays = np.ascontiguousarray(rays, np.float64)             # without the flag the library only reads them: no copy of 48 B per ray
        rays = rays.reshape(-1, 6)
        n = rays.shape[0]
        out = _result_array(out, n, parts[0]._slim_dtype() if slim else XEVENT_DTYPE)
        e1 = None if poly_origin1 is None else np.ascontiguousarray(poly_origin1, np.int32)
        e2 = None if poly_origin2 is None else np.ascontiguousarray(poly_origin2, np.int32)
        for e in (e1, e2):
            if e is not None and e.shape != (n,):
                raise ValueError("poly_origin arrays must have one entry per ray")
        handles = (C.c_void_p * len(parts))(*[p._h for p in parts])
        ctr = capi.Counters()
        check(lib.hare_shoot_batch_sharded(handles, len(parts), parts[0]._kind, int(top_index), n, ptr(rays), ptr(e1), ptr(e2),
                                           (capi.SHOOT_WRITEBACK_ORIGIN if writeback_origin else 0) | (capi.SHOOT_SLIM_EVENTS if slim else 0),
                                           ptr(out), C.addressof(ctr)))
        return out, ctr.as_dict()

    def Bounce_batch(self, rays, bounces: int, top_index: int = 0, poly_origin1=None, poly_origin2=None, all_casts: bool = False,
                     per_cast: bool = False, simple_kernel: bool = False, out=None):
        """The device-resident specular bounce loop from host buffers (hare_bounce_batch): `bounces` casts with a reflection
        between them, rays resident on the GPU throughout.  Returns (events, counters) -- events of the LAST cast [n], or with
        all_casts=True of every cast [bounces, n]; with per_cast=True a third value: the list of per-cast counter dicts."""
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        n, B = rays.shape[0], int(bounces)
        e1 = None if poly_origin1 is None else np.ascontiguousarray(poly_origin1, np.int32)
        e2 = None if poly_origin2 is None else np.ascontiguousarray(poly_origin2, np.int32)
        ev_all = _result_array(out, (B, n), XEVENT_DTYPE) if all_casts else None          # out: the caller's array, as in Shoot_batch
        ev_last = None if all_casts else _result_array(out, n, XEVENT_DTYPE)
        ctr = capi.Counters()
        pcs = (capi.Counters * max(B, 1))()
        check(lib.hare_bounce_batch(self._h, self._kind, int(top_index), n, ptr(rays), ptr(e1), ptr(e2), B,
                                    capi.SHOOT_SIMPLE_KERNEL if simple_kernel else 0, ptr(ev_all), ptr(ev_last), C.addressof(ctr),
                                    C.addressof(pcs)))
        out = (ev_all if all_casts else ev_last, ctr.as_dict())
        return out + ([pcs[b].as_dict() for b in range(B)],) if per_cast else out

    @staticmethod
    def Bounce_batch_sharded(partitions, rays, bounces: int, top_index: int = 0, all_casts: bool = False, out=None):
        """hare_bounce_batch_sharded: the loop over several devices from one process (contiguous ray shards, as Shoot_batch_sharded)."""
        parts = list(partitions)
        if not parts or any(p._kind != parts[0]._kind for p in parts):
            raise ValueError("need one or more partitions of the same kind")
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        n, B = rays.shape[0], int(bounces)
        ev_all = _result_array(out, (B, n), XEVENT_DTYPE) if all_casts else None          # out: the caller's array, as in Shoot_batch
        ev_last = None if all_casts else _result_array(out, n, XEVENT_DTYPE)
        handles = (C.c_void_p * len(parts))(*[p._h for p in parts])
        ctr = capi.Counters()
        check(lib.hare_bounce_batch_sharded(handles, len(parts), parts[0]._kind, int(top_index), n, ptr(rays), None, None, B, 0,
                                            ptr(ev_all), ptr(ev_last), C.addressof(ctr), None))
        return (ev_all if all_casts else ev_last), ctr.as_dict()

    # ---- receivers: energy-time histograms from the bounce loop (include/hare_hip.h, "receivers")
    def set_receivers(self, centers, radii):
        """hare_scene_set_receivers: K spheres, centers [K, 3], radii [K] (replaces the scene's receivers)."""
        c = np.ascontiguousarray(centers, np.float64).reshape(-1, 3)
        r = np.ascontiguousarray(radii, np.float64).reshape(-1)
        if r.shape[0] != c.shape[0]:
            raise ValueError("one radius per center")
        check(lib.hare_scene_set_receivers(self._h, c.shape[0], ptr(c), ptr(r)))
        return self

    def set_receiver_map(self, centers, radii, cell: float = 0.0):
        """hare_scene_set_receiver_map: up to 65 536 receivers, centers [K, 3], radii [K], found through a uniform grid over the centers
        (include/hare_hip.h, "Receiver maps").  cell: the grid's cell edge; 0 for the default, twice the largest radius.  Replaces the
        scene's receivers; set_receivers afterwards returns the scene to the linear loop."""
        c = np.ascontiguousarray(centers, np.float64).reshape(-1, 3)
        r = np.ascontiguousarray(radii, np.float64).reshape(-1)
        if r.shape[0] != c.shape[0]:
            raise ValueError("one radius per center")
        check(lib.hare_scene_set_receiver_map(self._h, c.shape[0], ptr(c), ptr(r), float(cell)))
        return self

    def receiver_map_info(self):
        """hare_scene_get_receiver_map: the grid of the scene's receiver map as a dict -- origin [3], cell (the edge h), pad (R), dims [3]
        (cells per axis, x fastest), cell_start [cells + 1] and cell_items [K] (CSR: each receiver in the cell of its center)."""
        geom, dims = np.zeros(5, np.float64), np.zeros(3, np.int32)
        check(lib.hare_scene_get_receiver_map(self._h, ptr(geom), ptr(dims), None, None))
        start = np.zeros(int(dims.prod(dtype=np.int64)) + 1, np.uint32)
        items = np.zeros(self.get_option("receivers"), np.uint32)
        check(lib.hare_scene_get_receiver_map(self._h, None, None, ptr(start), ptr(items)))
        return dict(origin=geom[:3].copy(), cell=float(geom[3]), pad=float(geom[4]), dims=dims, cell_start=start, cell_items=items)

    @staticmethod
    def receiver_plane(lo, hi, height: float, spacing: float, radius: float):
        """A map's layout: receivers on the plane z = height, `spacing` apart in x and y, centred in the rectangle lo .. hi (two points;
        their x and y are read).  Returns (centers [K, 3], radii [K]) for set_receiver_map."""
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        axes = []
        for a in range(2):
            cnt = max(1, int(np.floor((hi[a] - lo[a]) / spacing)) + 1)
            first = 0.5 * ((lo[a] + hi[a]) - (cnt - 1) * spacing)
            axes.append(first + spacing * np.arange(cnt))
        x, y = np.meshgrid(axes[0], axes[1], indexing="xy")
        c = np.stack([x.ravel(), y.ravel(), np.full(x.size, float(height))], axis=1)
        return np.ascontiguousarray(c), np.full(c.shape[0], float(radius))

    def set_absorption(self, alpha, top_index: int = 0):
        """hare_scene_set_absorption: alpha [P, B] in [0, 1] for Model[top_index] (B = 1 .. 8 bands)."""
        a = np.ascontiguousarray(alpha, np.float64)
        if a.ndim != 2:
            raise ValueError("alpha must be [polygons, bands]")
        check(lib.hare_scene_set_absorption(self._h, int(top_index), a.shape[1], ptr(a)))
        return self

    def set_scattering(self, sigma, top_index: int = 0):
        """hare_scene_set_scattering: sigma [P, B] in [0, 1] for Model[top_index] (the same B as its absorption table, if any): the receive
        loop scatters diffusely (seed: option "scatter_seed").  sigma None removes the table (specular reflection only)."""
        if sigma is None:
            check(lib.hare_scene_set_scattering(self._h, int(top_index), 0, None))
            return self
        s = np.ascontiguousarray(sigma, np.float64)
        if s.ndim != 2:
            raise ValueError("sigma must be [polygons, bands]")
        check(lib.hare_scene_set_scattering(self._h, int(top_index), s.shape[1], ptr(s)))
        return self

    def set_source(self, pos, power=None, frame=None, gain=None):
        """hare_scene_set_source: the scene's point source (include/hare_hip.h, "receivers", "Source").  pos [3]; power [B] per band (None:
        1.0 in each of the B bands of `gain`, or of topology 0 without a table); frame [3, 3] (None: identity); gain [6, R, R, B], the
        directivity as a nearest-texel cube map read in the source's frame (None: omnidirectional).  Seed: option "source_seed"."""
        p = np.ascontiguousarray(pos, np.float64).reshape(-1)
        if p.shape != (3,):
            raise ValueError("pos must be [3]")
        g = None if gain is None else np.ascontiguousarray(gain, np.float64)
        if g is not None and not (g.ndim == 4 and g.shape[0] == 6 and g.shape[1] == g.shape[2]):
            raise ValueError("gain must be [6, R, R, B]")
        w = None if power is None else np.ascontiguousarray(power, np.float64).reshape(-1)
        B = w.shape[0] if w is not None else (g.shape[3] if g is not None else self._bands(0))
        if g is not None and g.shape[3] != B:
            raise ValueError("power and gain must have the same number of bands")
        f = None if frame is None else np.ascontiguousarray(frame, np.float64).reshape(-1)
        if f is not None and f.shape != (9,):
            raise ValueError("frame must be [3, 3]")
        check(lib.hare_scene_set_source(self._h, ptr(p), int(B), ptr(w), ptr(f), 0 if g is None else g.shape[1], ptr(g)))
        return self

    def set_edges(self, ends, faces, inv_lambda, top_index: int = 0):
        """hare_scene_set_edges: the diffracting edges of Model[top_index] (include/hare_hip.h, "receivers", "Edge diffraction (first
        order)").  ends [E, 2, 3] (or [E, 6]): a and b of every edge; faces int32 [E, 2]: the polygons that meet in it, -1 for none;
        inv_lambda [B]: f_b / c per band (hare_amd.edges.band_inv_lambda).  hare_amd.edges.find_edges proposes ends and faces from a
        topology.  ends None removes the table."""
        if ends is None:
            check(lib.hare_scene_set_edges(self._h, int(top_index), 0, None, None, 0, None))
            return self
        e = np.ascontiguousarray(ends, np.float64).reshape(-1, 6)
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 2)
        w = np.ascontiguousarray(inv_lambda, np.float64).reshape(-1)
        if f.shape[0] != e.shape[0]:
            raise ValueError("one pair of faces per edge")
        check(lib.hare_scene_set_edges(self._h, int(top_index), e.shape[0], ptr(e), ptr(f), w.shape[0], ptr(w)))
        return self

    def emit_device(self, n: int, d_rays: int, d_state: int, first_ray: int = 0, stream: int = 0):
        """hare_emit_device on raw device addresses + a hipStream_t: the source's rays first_ray .. first_ray + n - 1 into d_rays (n x 48 B)
        and their state into d_state ((1 + B) x n doubles, B = get_option("source_bands")).  Stream-ordered."""
        check(lib.hare_emit_device(self._h, int(n), int(first_ray), d_rays or None, d_state or None, stream or None))

    def Receive_source(self, n: int, bounces: int, n_bins: int, bin_len: float, first_ray: int = 0, frac_bits: int = 40, top_index: int = 0,
                       out=None, rain: bool = False, directional: bool = False, time_limit: bool = False, direct: bool = False,
                       image: bool = False, image2: bool = False, *, order: int = 1):
        """hare_receive_source: Receive_batch with the rays and their state emitted on the device by the scene's source (set_source) --
        the rays first_ray .. first_ray + n - 1; nothing but the count goes up.  Returns what Receive_batch returns.  Calls over
        [0, k) and [k, n) sum to the histogram and detections of the one call.  direct (HARE_RECEIVE_DIRECT; include/hare_hip.h, "Direct
        sound"): the direct sound is one visibility-tested deposit per receiver, standing for the call's n rays, and cast 0 detects
        nothing -- chunks then sum to the one call up to a unit per chunk and word.  image (HARE_RECEIVE_IMAGE; "Image sources (first
        order)"): the first-order specular reflections are one visibility-tested deposit per (receiver, polygon) pair, and in cast 1 the
        rays that left cast 0 specularly detect nothing; the pair list holds get_option("image_max_pairs") pairs (HareError, HARE_E_NOMEM,
        with the needed count when the scene yields more).  image2 (HARE_RECEIVE_IMAGE2, only with image; "Image sources (second
        order)"): the specular paths off two polygons are one deposit each, and in cast 2 the rays reflected specularly twice detect nothing;
        the lists hold get_option("image2_max_cands") candidates and get_option("image2_max_paths") paths (HARE_E_NOMEM with both counts).
        order (with directional; HARE_RECEIVE_ORDER2 / _ORDER3, "Higher orders"): 2 or 3 widens the histogram to 9 or 16 channels."""
        return Spatial_Partition._receive_source([self], n, bounces, n_bins, bin_len, first_ray, frac_bits, top_index, out, rain, directional,
                                                 time_limit, direct=direct, image=image, image2=image2, order=order)

    def Receive_source_reduced(self, n: int, bounces: int, n_bins: int, bin_len: float, windows=None, levels=None, weight=None,
                               first_ray: int = 0, frac_bits: int = 40, top_index: int = 0, directional: bool = False,
                               time_limit: bool = False, direct: bool = False, image: bool = False, image2: bool = False, *, order: int = 1):
        """hare_receive_source_reduced: Receive_source with the histogram kept on the device and reduced there, as in
        Receive_batch_reduced; returns what that returns.  direct, image: as in Receive_source."""
        return Spatial_Partition._receive_source([self], n, bounces, n_bins, bin_len, first_ray, frac_bits, top_index, None, False, directional,
                                                 time_limit, dict(windows=windows, levels=levels, weight=weight), direct=direct, image=image, image2=image2,
                                                 order=order)

    @staticmethod
    def Receive_source_sharded(partitions, n: int, bounces: int, n_bins: int, bin_len: float, first_ray: int = 0, frac_bits: int = 40,
                               top_index: int = 0, out=None, rain: bool = False, directional: bool = False, time_limit: bool = False,
                               direct: bool = False, image: bool = False, image2: bool = False, *, order: int = 1):
        """hare_receive_source_sharded: Receive_source over several partitions (contiguous ray shards, histograms summed); byte-identical.
        The partitions must hold the same source and "source_seed".  direct, image: as in Receive_source; one partition makes each deposit."""
        return Spatial_Partition._receive_source(list(partitions), n, bounces, n_bins, bin_len, first_ray, frac_bits, top_index, out, rain,
                                                 directional, time_limit, direct=direct, image=image, image2=image2, order=order)

    @staticmethod
    def _receive_source(parts, n, bounces, n_bins, bin_len, first_ray, frac_bits, top_index, out, rain, directional, time_limit, reduce=None,
                        direct=False, image=False, image2=False, order=1):
        if not parts or any(p._kind != parts[0]._kind for p in parts):
            raise ValueError("need one or more partitions of the same kind")
        n = int(n)
        if n < 0:
            raise ValueError("n must be >= 0")
        shape = parts[0]._receive_shape(top_index, n_bins, bool(directional), order=order)
        K, nb, B = shape[:3]
        det = np.zeros((max(K, 0), 2), np.uint64)
        state_out = np.empty((1 + B, n), np.float64)
        ctr = capi.Counters()
        flags = ((capi.RECEIVE_DIFFUSE_RAIN if rain else 0) | capi.channel_flags(directional, order) |
                 (capi.RECEIVE_TIME_LIMIT if time_limit else 0) | (capi.RECEIVE_DIRECT if direct else 0) |
                 (capi.RECEIVE_IMAGE if image else 0) | (capi.RECEIVE_IMAGE2 if image2 else 0))
        if reduce is not None:
            w, n_win, win, n_lev, lev = _reduce_spec(reduce, nb, B)
            sums, cross = np.zeros((max(K, 0), B, n_win, 4), np.uint64), np.zeros((max(K, 0), B, n_lev), np.int32)
            check(lib.hare_receive_source_reduced(parts[0]._h, parts[0]._kind, int(top_index), n, int(first_ray), int(bounces), flags, nb,
                                                  float(bin_len), int(frac_bits), ptr(state_out), ptr(w), n_win, ptr(win), n_lev, ptr(lev),
                                                  ptr(sums), ptr(cross), ptr(det), C.addressof(ctr)))
            return sums, cross, det, state_out, ctr.as_dict()
        hist = _result_array(out, (max(K, 0),) + shape[1:], np.uint64)
        if len(parts) == 1:
            rc = lib.hare_receive_source(parts[0]._h, parts[0]._kind, int(top_index), n, int(first_ray), int(bounces), flags, nb, float(bin_len),
                                         int(frac_bits), ptr(state_out), ptr(hist), ptr(det), C.addressof(ctr))
        else:
            handles = (C.c_void_p * len(parts))(*[p._h for p in parts])
            rc = lib.hare_receive_source_sharded(handles, len(parts), parts[0]._kind, int(top_index), n, int(first_ray), int(bounces), flags, nb,
                                                 float(bin_len), int(frac_bits), ptr(state_out), ptr(hist), ptr(det), C.addressof(ctr))
        check(rc)
        return hist, hist.astype(np.float64) * 2.0 ** -int(frac_bits), det, state_out, ctr.as_dict()

    def _receive_shape(self, top_index: int, n_bins: int, directional: bool = False, *, order: int = 1):
        shape = (self.get_option("receivers"), int(n_bins), self._bands(top_index))
        capi.channel_flags(directional, order)                      # ValueError for an order that is none
        return shape + (capi.ORDER_CHANNELS[int(order)],) if directional else shape

    @staticmethod
    def directional_signed(hist):
        """The signed channels of a directional histogram [K, n_bins, B, C], C = 4, 9 or 16 (order 1, 2, 3): channels 1 .. C - 1 as int64
        [K, n_bins, B, C - 1] (a view, no copy).  Channel 0 is W, the omni word a call without `directional` returns; channels 1, 2, 3
        are X, Y, Z in world axes, positive for sound ARRIVING FROM +x, +y, +z (the ambisonic sign convention), in two's complement at
        the same scale 2^-frac_bits; channels 4 .. C - 1 are ACN 4 .. C - 1 in SN3D ("Higher orders")."""
        hist = np.asarray(hist)
        if hist.dtype != np.uint64 or hist.ndim < 1 or hist.shape[-1] not in (4, 9, 16):
            raise ValueError("need a directional histogram: uint64 [..., 4], [..., 9] or [..., 16]")
        return hist[..., 1:].view(np.int64)

    def _bands(self, top_index: int) -> int:
        return self.get_option("bands:%d" % int(top_index))          # the scene's own record, whoever set the table

    def Receive_batch(self, rays, bounces: int, n_bins: int, bin_len: float, energy=None, frac_bits: int = 40, top_index: int = 0,
                      poly_origin1=None, poly_origin2=None, out=None, rain: bool = False, directional: bool = False, time_limit: bool = False,
                      *, order: int = 1):
        """The bounce loop with the receiver step between its casts, from host buffers (hare_receive_batch).
        energy: None (every ray starts at L = 0, E = 1) or the state [1 + B, n] (row 0: L, rows 1..B: E).
        Returns (hist [K, n_bins, B] uint64, hist * 2^-frac_bits as float64, detections [K, 2] uint64, final state [1 + B, n],
        counters).  out (optional): the caller's uint64 histogram array [K, n_bins, B], as in Shoot_batch.  rain: diffuse rain
        (HARE_RECEIVE_DIFFUSE_RAIN) where the topology has a scattering table.  directional (HARE_RECEIVE_DIRECTIONAL): the histogram
        (and `out`) is [K, n_bins, B, 4], channels W, X, Y, Z (directional_signed gives X, Y, Z as int64); frac_bits must leave a sign
        bit of headroom; order 2 or 3 with it (HARE_RECEIVE_ORDER2 / _ORDER3): [K, n_bins, B, 9] or [K, n_bins, B, 16], the channels
        of "Higher orders" behind the four.  time_limit (HARE_RECEIVE_TIME_LIMIT): a ray whose path L has reached n_bins * bin_len after a hit is retired;
        histogram and detections[:, 0] stay as they are without it.  The energy floor is the scene's: options "receive_floor_bits"
        (F = 2^-f) and "receive_roulette" (include/hare_hip.h, "Termination")."""
        return Spatial_Partition._receive([self], rays, bounces, n_bins, bin_len, energy, frac_bits, top_index, poly_origin1,
                                          poly_origin2, out, rain, directional, time_limit, order=order)

    def Receive_batch_reduced(self, rays, bounces: int, n_bins: int, bin_len: float, windows=None, levels=None, weight=None, energy=None,
                              frac_bits: int = 40, top_index: int = 0, poly_origin1=None, poly_origin2=None, directional: bool = False,
                              time_limit: bool = False, *, order: int = 1):
        """hare_receive_batch_reduced (include/hare_hip.h, "receivers", "Reduction"): Receive_batch with the histogram kept on the device
        and reduced there.  windows: [(lo, hi), ...] bin ranges; levels: uint32 fractions (decay_levels); weight: uint32 [n_bins, B]
        (air_weights) or None.  Returns (sums [K, B, n_win, 4] uint64 -- S0 lo, S0 hi, S1 lo, S1 hi --, cross [K, B, n_lev] int32,
        detections, final state, counters): sums and cross are hist_reduce of the histogram Receive_batch returns."""
        return Spatial_Partition._receive([self], rays, bounces, n_bins, bin_len, energy, frac_bits, top_index, poly_origin1, poly_origin2,
                                          None, False, directional, time_limit, dict(windows=windows, levels=levels, weight=weight), order=order)

    @staticmethod
    def Receive_batch_sharded(partitions, rays, bounces: int, n_bins: int, bin_len: float, energy=None, frac_bits: int = 40,
                              top_index: int = 0, poly_origin1=None, poly_origin2=None, out=None, rain: bool = False,
                              directional: bool = False, time_limit: bool = False, *, order: int = 1):
        """hare_receive_batch_sharded: Receive_batch over several partitions (contiguous ray shards, histograms summed); byte-identical.
        The partitions must agree in "receive_floor_bits" and "receive_roulette" (and, with roulette, in "scatter_seed")."""
        return Spatial_Partition._receive(list(partitions), rays, bounces, n_bins, bin_len, energy, frac_bits, top_index, poly_origin1,
                                          poly_origin2, out, rain, directional, time_limit, order=order)

    @staticmethod
    def _receive(parts, rays, bounces, n_bins, bin_len, energy, frac_bits, top_index, poly_origin1, poly_origin2, out, rain=False, directional=False,
                 time_limit=False, reduce=None, order=1):
        if not parts or any(p._kind != parts[0]._kind for p in parts):
            raise ValueError("need one or more partitions of the same kind")
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        n = rays.shape[0]
        shape = parts[0]._receive_shape(top_index, n_bins, bool(directional), order=order)      # [K, n_bins, B], and the channels with the flag
        K, nb, B = shape[:3]
        e1 = None if poly_origin1 is None else np.ascontiguousarray(poly_origin1, np.int32)
        e2 = None if poly_origin2 is None else np.ascontiguousarray(poly_origin2, np.int32)
        for e in (e1, e2):
            if e is not None and e.shape != (n,):
                raise ValueError("poly_origin arrays must have one entry per ray")
        state_in = None
        if energy is not None:
            state_in = np.ascontiguousarray(energy, np.float64)
            if state_in.shape != (1 + B, n):
                raise ValueError("energy must be the state [1 + B, n] = [%d, %d]" % (1 + B, n))
        det = np.zeros((max(K, 0), 2), np.uint64)
        state_out = np.empty((1 + B, n), np.float64)
        ctr = capi.Counters()
        flags = ((capi.RECEIVE_DIFFUSE_RAIN if rain else 0) | capi.channel_flags(directional, order) |
                 (capi.RECEIVE_TIME_LIMIT if time_limit else 0))
        if reduce is not None:
            w, n_win, win, n_lev, lev = _reduce_spec(reduce, nb, B)
            sums, cross = np.zeros((max(K, 0), B, n_win, 4), np.uint64), np.zeros((max(K, 0), B, n_lev), np.int32)
            check(lib.hare_receive_batch_reduced(parts[0]._h, parts[0]._kind, int(top_index), n, ptr(rays), ptr(e1), ptr(e2), int(bounces), flags,
                                                 nb, float(bin_len), int(frac_bits), ptr(state_in), ptr(state_out), ptr(w), n_win, ptr(win),
                                                 n_lev, ptr(lev), ptr(sums), ptr(cross), ptr(det), C.addressof(ctr)))
            return sums, cross, det, state_out, ctr.as_dict()
        hist = _result_array(out, (max(K, 0),) + shape[1:], np.uint64)
        if len(parts) == 1:
            rc = lib.hare_receive_batch(parts[0]._h, parts[0]._kind, int(top_index), n, ptr(rays), ptr(e1), ptr(e2), int(bounces), flags, nb,
                                        float(bin_len), int(frac_bits), ptr(state_in), ptr(state_out), ptr(hist), ptr(det), C.addressof(ctr))
        else:
            handles = (C.c_void_p * len(parts))(*[p._h for p in parts])
            rc = lib.hare_receive_batch_sharded(handles, len(parts), parts[0]._kind, int(top_index), n, ptr(rays), ptr(e1), ptr(e2),
                                                int(bounces), flags, nb, float(bin_len), int(frac_bits), ptr(state_in), ptr(state_out),
                                                ptr(hist), ptr(det), C.addressof(ctr))
        check(rc)
        return hist, hist.astype(np.float64) * 2.0 ** -int(frac_bits), det, state_out, ctr.as_dict()

    def hist_reduce(self, hist, windows=None, levels=None, weight=None):
        """hare_hist_reduce: a histogram [K, n_bins, B] (or [K, n_bins, B, C], directional with C = 4, 9 or 16: channel 0 is read) of uint64, as the receive
        calls return it, reduced on this partition's device (include/hare_hip.h, "receivers", "Reduction").  windows: [(lo, hi), ...] bin
        ranges; levels: uint32 fractions (decay_levels); weight: uint32 [n_bins, B] (air_weights) or None.  Returns (sums [K, B, n_win, 4]
        uint64 -- S0 lo, S0 hi, S1 lo, S1 hi --, cross [K, B, n_lev] int32)."""
        hist, K, nb, B, channels = _hist_shape(hist)
        w, n_win, win, n_lev, lev = _reduce_spec(dict(windows=windows, levels=levels, weight=weight), nb, B)
        sums, cross = np.zeros((K, B, n_win, 4), np.uint64), np.zeros((K, B, n_lev), np.int32)
        check(lib.hare_hist_reduce(self._h, K, nb, B, channels, ptr(hist), ptr(w), n_win, ptr(win), n_lev, ptr(lev),
                                   ptr(sums), ptr(cross)))
        return sums, cross

    def hist_reduce_device(self, K: int, n_bins: int, B: int, channels: int, d_hist: int, d_sums: int, d_cross: int, windows=None,
                           levels=None, d_weight: int = 0, stream: int = 0):
        """hare_hist_reduce_device on raw device addresses + a hipStream_t: d_hist as receive_device accumulates it, d_sums (K x B x n_win
        x 4 uint64) and d_cross (K x B x n_lev int32) written, d_weight (n_bins x B uint32) or 0.  windows and levels are host data, read
        at the call.  Stream-ordered: no allocation, no free, no wait."""
        _, n_win, win, n_lev, lev = _reduce_spec(dict(windows=windows, levels=levels), n_bins, B)
        check(lib.hare_hist_reduce_device(self._h, int(K), int(n_bins), int(B), int(channels), d_hist or None, d_weight or None, n_win,
                                          ptr(win), n_lev, ptr(lev), d_sums or None, d_cross or None, stream or None))

    def hist_project(self, hist, coef, weight=None, as_int: bool = False):
        """hare_hist_project: a histogram [K, n_bins, B] or [K, n_bins, B, C] (C = 4, 9 or 16: channel 0 is read) of uint64, as the receive
        calls return it, projected on this partition's device onto the vectors coef, int32 [J, n_bins] with 1 <= J <= 32 (include/hare_hip.h,
        "receivers", "Projection"): the exact signed sums over the bins of coef[j, i] * g[k, i, b].  weight: uint32 [n_bins, B] (air_weights)
        or None.  Returns uint64 [K, B, J, 2], the (lo, hi) words of the 128-bit two's-complement sums, or with as_int an object array
        [K, B, J] of Python integers (proj_to_int)."""
        hist, K, nb, B, channels = _hist_shape(hist)
        coef = _project_coef(coef, nb)
        w, *_ = _reduce_spec(dict(weight=weight), nb, B)
        proj = np.zeros((K, B, coef.shape[0], 2), np.uint64)
        check(lib.hare_hist_project(self._h, K, nb, B, channels, ptr(hist), ptr(w), coef.shape[0], ptr(coef),
                                    ptr(proj)))
        return proj_to_int(proj) if as_int else proj

    def hist_project_device(self, K: int, n_bins: int, B: int, channels: int, d_hist: int, J: int, d_coef: int, d_proj: int, d_weight: int = 0,
                            stream: int = 0):
        """hare_hist_project_device on raw device addresses + a hipStream_t: d_hist as receive_device accumulates it, d_coef (J x n_bins
        int32), d_proj (K x B x J x 2 uint64) written, d_weight (n_bins x B uint32) or 0.  Stream-ordered: no allocation, no free, no wait,
        no upload."""
        check(lib.hare_hist_project_device(self._h, int(K), int(n_bins), int(B), int(channels), d_hist or None, d_weight or None, int(J),
                                           d_coef or None, d_proj or None, stream or None))

    def hist_project_channels(self, hist, coef, weight=None, as_int: bool = False):
        """hare_hist_project_channels: hist_project for EVERY channel of a histogram [K, n_bins, B] or [K, n_bins, B, C] (C = 4, 9 or 16) of
        uint64 (include/hare_hip.h, "receivers", "Directional projection"): channel 0 unsigned, the channels after it two's-complement
        int64, weighted with a floor towards minus infinity.  coef: int32 [J, n_bins], 1 <= J <= 32; weight: uint32 [n_bins, B]
        (air_weights) or None.  Returns uint64 [K, B, J, C, 2], the (lo, hi) words of the exact 128-bit two's-complement sums over the bins
        of coef[j, i] * g[k, i, b, ch], or with as_int an object array [K, B, J, C] of Python integers (proj_to_int).  hare_amd.spatial
        turns them into the intensity vector, the second moments and the lateral fraction."""
        hist, K, nb, B, channels = _hist_shape(hist)
        coef = _project_coef(coef, nb)
        w, *_ = _reduce_spec(dict(weight=weight), nb, B)
        proj = np.zeros((K, B, coef.shape[0], channels, 2), np.uint64)
        check(lib.hare_hist_project_channels(self._h, K, nb, B, channels, ptr(hist), ptr(w), coef.shape[0], ptr(coef), ptr(proj)))
        return proj_to_int(proj) if as_int else proj

    def hist_project_channels_device(self, K: int, n_bins: int, B: int, channels: int, d_hist: int, J: int, d_coef: int, d_proj: int,
                                     d_weight: int = 0, stream: int = 0):
        """hare_hist_project_channels_device on raw device addresses + a hipStream_t: d_hist as receive_device accumulates it, d_coef
        (J x n_bins int32), d_proj (K x B x J x channels x 2 uint64) written, d_weight (n_bins x B uint32) or 0.  Stream-ordered: no
        allocation, no free, no wait, no upload."""
        check(lib.hare_hist_project_channels_device(self._h, int(K), int(n_bins), int(B), int(channels), d_hist or None, d_weight or None,
                                                    int(J), d_coef or None, d_proj or None, stream or None))

    def hist_render(self, hist, taps, M: int, frac_bits: int, seed: int = 0, weight=None):
        """hare_hist_render: a histogram [K, n_bins, B] or [K, n_bins, B, C] (C = 4, 9 or 16) of uint64, as the receive calls return it,
        rendered on this partition's device to impulse responses (include/hare_hip.h, "receivers", "Rendering"): M samples per bin, taps
        [B, T] float64 (band_taps), seed uint64, weight uint32 [n_bins, B] (air_weights) or None.  Returns float64 [K, channels, n_bins * M]."""
        hist, K, nb, B, channels = _hist_shape(hist)
        taps = np.ascontiguousarray(taps, np.float64)
        if taps.ndim != 2 or taps.shape[0] != B:
            raise ValueError("taps must be float64 [B, T] = [%d, T]" % B)
        w, *_ = _reduce_spec(dict(weight=weight), nb, B)
        out = np.zeros((K, channels, nb * max(0, int(M))), np.float64)
        check(lib.hare_hist_render(self._h, K, nb, B, channels, ptr(hist), ptr(w), int(frac_bits), int(M), taps.shape[1], ptr(taps),
                                   int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(out)))
        return out

    def hist_render_device(self, K: int, n_bins: int, B: int, channels: int, d_hist: int, frac_bits: int, M: int, T: int, d_taps: int,
                           seed: int, d_out: int, d_weight: int = 0, stream: int = 0):
        """hare_hist_render_device on raw device addresses + a hipStream_t: d_hist as receive_device accumulates it, d_taps (B x T float64),
        d_out (K x channels x n_bins x M float64) written, d_weight (n_bins x B uint32) or 0.  Stream-ordered: no allocation, no free, no
        wait."""
        check(lib.hare_hist_render_device(self._h, int(K), int(n_bins), int(B), int(channels), d_hist or None, d_weight or None, int(frac_bits),
                                          int(M), int(T), d_taps or None, int(seed) & 0xFFFFFFFFFFFFFFFF, d_out or None, stream or None))

    def hist_impulses(self, hist, taps, frac_bits: int, n0: int = 0, n_out=None, weight=None, out=None):
        """hare_hist_impulses: a PER-SAMPLE histogram [K, n_bins, B] or [K, n_bins, B, C] (C = 4, 9 or 16) of uint64 -- Source_paths with
        bin_len = c / fs -- turned on this partition's device into pressure rows (include/hare_hip.h, "receivers", "Impulses"): every
        non-empty (bin, band) an impulse of amplitude sqrt(energy) through that band's row of taps [B, T] float64, weighted per channel by
        the rendering's ratio.  The window [n0, n0 + n_out) of the n_bins + T - 1 samples is computed; n_out None: everything from n0 on.
        weight uint32 [n_bins, B] (air_weights) or None.  out None: returns a new float64 [K, channels, n_out].  out given, float64
        [K, channels, stride] C-contiguous with stride >= n_out: the impulses are ADDED onto its first n_out samples per row (add = 1; e.g.
        what hist_render returned), the rest is left as it is, and out is returned."""
        hist, K, nb, B, channels = _hist_shape(hist)
        taps = np.ascontiguousarray(taps, np.float64)
        if taps.ndim != 2 or taps.shape[0] != B or taps.shape[1] < 1:
            raise ValueError("taps must be float64 [B, T] = [%d, T]" % B)
        w, *_ = _reduce_spec(dict(weight=weight), nb, B)
        T, n0 = taps.shape[1], int(n0)
        n_out = nb + T - 1 - n0 if n_out is None else int(n_out)
        add = 0 if out is None else 1
        if out is None:
            out = np.zeros((K, channels, max(0, n_out)), np.float64)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous and out.flags.writeable
                  and out.ndim == 3 and out.shape[:2] == (K, channels)):
            raise ValueError("out must be a writeable C-contiguous float64 [K, channels, stride] = [%d, %d, stride]" % (K, channels))
        check(lib.hare_hist_impulses(self._h, K, nb, B, channels, ptr(hist), ptr(w), int(frac_bits), T, ptr(taps), n0, n_out, out.shape[2], add,
                                     ptr(out)))
        return out

    def hist_impulses_device(self, K: int, n_bins: int, B: int, channels: int, d_hist: int, frac_bits: int, T: int, d_taps: int, n0: int,
                             n_out: int, out_stride: int, add: int, d_out: int, d_weight: int = 0, stream: int = 0):
        """hare_hist_impulses_device on raw device addresses + a hipStream_t: d_hist as direct_device / image_device / image2_device
        accumulate it with a bin of one sample, d_taps (B x T float64), d_out (K x channels x out_stride float64): the first n_out words of
        each row written (add 0) or added onto (add 1).  d_weight (n_bins x B uint32) or 0.  Stream-ordered: no allocation, no free, no wait."""
        check(lib.hare_hist_impulses_device(self._h, int(K), int(n_bins), int(B), int(channels), d_hist or None, d_weight or None, int(frac_bits),
                                            int(T), d_taps or None, int(n0), int(n_out), int(out_stride), int(add), d_out or None, stream or None))

    def Source_paths(self, n_weight: int, n_bins: int, bin_len: float, frac_bits: int = 40, top_index: int = 0, directional: bool = False,
                     direct: bool = True, image: bool = True, image2: bool = True, *, order: int = 1):
        """hare_source_paths: the deterministic paths of the scene's source alone -- the direct sound (direct), the first-order image sources
        (image) and the second-order ones (image2, only with image) -- deposited into a zeroed histogram, each standing for n_weight rays:
        what Receive_source deposits ahead of cast 0 under the same flags, and nothing of the loop.  With bin_len = c / fs the histogram is
        what hist_impulses takes.  Returns (hist uint64 [K, n_bins, B] or [K, n_bins, B, C], detections uint64 [K, 2])."""
        shape = self._receive_shape(top_index, n_bins, bool(directional), order=order)
        K = max(shape[0], 0)
        hist, det = np.zeros((K,) + shape[1:], np.uint64), np.zeros((K, 2), np.uint64)
        flags = (capi.channel_flags(directional, order) | (capi.RECEIVE_DIRECT if direct else 0) | (capi.RECEIVE_IMAGE if image else 0) |
                 (capi.RECEIVE_IMAGE2 if image2 else 0))
        check(lib.hare_source_paths(self._h, self._kind, int(top_index), int(n_weight), flags, int(n_bins), float(bin_len), int(frac_bits),
                                    ptr(hist), ptr(det)))
        return hist, det

    def convolve(self, ir, x, n0: int = 0, n_out=None):
        """hare_convolve: the rows of ir -- float64 [R, N], or [K, C, N] as hist_render returns it (row k * C + ch) -- each convolved on
        this partition's device with the one signal x, float64 [L] (include/hare_hip.h, "receivers", "Convolution"): FP64 in the time
        domain, every output one sequential sum over its taps.  The window [n0, n0 + n_out) of the N + L - 1 samples of the full convolution
        is computed; n_out None: everything from n0 on.  Returns float64 [R, n_out]."""
        ir, x = np.ascontiguousarray(ir, np.float64), np.ascontiguousarray(x, np.float64)
        if ir.ndim not in (2, 3) or ir.size == 0:
            raise ValueError("ir must be float64 [R, N] or [K, C, N], not empty")
        if x.ndim != 1 or x.size == 0:
            raise ValueError("x must be float64 [L], not empty")
        ir = ir.reshape(-1, ir.shape[-1])
        R, N, L = ir.shape[0], ir.shape[1], x.shape[0]
        n0 = int(n0)
        n_out = N + L - 1 - n0 if n_out is None else int(n_out)
        y = np.zeros((R, max(0, n_out)), np.float64)
        check(lib.hare_convolve(self._h, R, N, ptr(ir), L, ptr(x), n0, n_out, ptr(y)))
        return y

    def convolve_device(self, R: int, N: int, d_ir: int, L: int, d_x: int, n0: int, n_out: int, d_y: int, stream: int = 0):
        """hare_convolve_device on raw device addresses + a hipStream_t: d_ir (R x N float64, e.g. hist_render_device's d_out with
        R = K x channels), d_x (L float64), d_y (R x n_out float64) written.  Stream-ordered: no allocation, no free, no wait."""
        check(lib.hare_convolve_device(self._h, int(R), int(N), d_ir or None, int(L), d_x or None, int(n0), int(n_out), d_y or None,
                                       stream or None))

    def decode(self, in_, h, n0: int = 0, n_out=None):
        """hare_decode: the rows of in_ -- float64 [K, C, N], as hist_render returns it: ambisonic channels per receiver -- decoded on this
        partition's device through the matrix of FIR filters h, float64 [O, C, T] (include/hare_hip.h, "receivers", "Decoding"): output
        (k, o) is the sum over all channels c of in_[k, c] filtered by h[o, c], FP64 in the time domain, every output one sequential sum
        over c and, within c, over the taps.  The window [n0, n0 + n_out) of the N + T - 1 samples is computed; n_out None: everything
        from n0 on.  Returns float64 [K, O, n_out].  hare_amd.decoders builds h for loudspeakers and for a caller's HRIR set."""
        in_, h = np.ascontiguousarray(in_, np.float64), np.ascontiguousarray(h, np.float64)
        if in_.ndim != 3 or in_.size == 0:
            raise ValueError("in_ must be float64 [K, C, N], not empty")
        if h.ndim != 3 or h.size == 0:
            raise ValueError("h must be float64 [O, C, T], not empty")
        if h.shape[1] != in_.shape[1]:
            raise ValueError("h [O, C, T] must have the C of in_ [K, C, N]")
        (K, Cn, N), (O, _, T) = in_.shape, h.shape
        n0 = int(n0)
        n_out = N + T - 1 - n0 if n_out is None else int(n_out)
        y = np.zeros((K, O, max(0, n_out)), np.float64)
        check(lib.hare_decode(self._h, K, Cn, N, ptr(in_), O, T, ptr(h), n0, n_out, ptr(y)))
        return y

    def decode_device(self, K: int, C: int, N: int, d_in: int, O: int, T: int, d_h: int, n0: int, n_out: int, d_y: int, stream: int = 0):
        """hare_decode_device on raw device addresses + a hipStream_t: d_in (K x C x N float64, e.g. hist_render_device's d_out with
        C = channels), d_h (O x C x T float64), d_y (K x O x n_out float64) written.  Stream-ordered: no allocation, no free, no wait."""
        check(lib.hare_decode_device(self._h, int(K), int(C), int(N), d_in or None, int(O), int(T), d_h or None, int(n0), int(n_out),
                                     d_y or None, stream or None))

    @staticmethod
    def direct_work_bytes(K: int) -> int:
        """Bytes of direct_device's d_work for K receivers: HARE_DIRECT_WORK_BYTES(K)."""
        return 64 * int(K) + 256

    def direct_device(self, n_weight: int, n_bins: int, bin_len: float, frac_bits: int, d_work: int, d_hist: int, d_detections: int,
                      top_index: int = 0, directional: bool = False, stream: int = 0, *, order: int = 1):
        """hare_direct_device on raw device addresses + a hipStream_t: the direct sound of the scene's source (include/hare_hip.h, "Direct
        sound") -- one visibility query and one deposit per receiver, standing for n_weight source rays -- accumulated into d_hist
        (K x n_bins x B uint64, x 4 with directional, x 9 or x 16 with order 2 or 3 beside it) and d_detections (2 K uint64); d_work holds
        direct_work_bytes(K) bytes.
        Stream-ordered: no allocation, no free, no wait."""
        check(lib.hare_direct_device(self._h, self._kind, int(top_index), int(n_weight), capi.channel_flags(directional, order),
                                     int(n_bins), float(bin_len), int(frac_bits), d_work or None, d_hist or None, d_detections or None,
                                     stream or None))

    @staticmethod
    def image_work_bytes(K: int, P: int, max_pairs: int) -> int:
        """Bytes of Image_device's d_work for K receivers, P polygons and a list of max_pairs pairs: HARE_IMAGE_WORK_BYTES(K, P, max_pairs)."""
        return 256 + 32 * int(P) + 136 * int(max_pairs)

    def Image_device(self, n_weight: int, n_bins: int, bin_len: float, frac_bits: int, max_pairs: int, d_work: int, d_hist: int,
                     d_detections: int, top_index: int = 0, directional: bool = False, stream: int = 0, *, order: int = 1):
        """hare_image_device on raw device addresses + a hipStream_t: the first-order image sources of the scene's source
        (include/hare_hip.h, "Image sources (first order)") -- the pair search receivers x polygons, two shadow rays per accepted pair and
        one deposit per pair with both legs free, standing for n_weight source rays -- accumulated into d_hist (K x n_bins x B uint64,
        x 4 with directional, x 9 or x 16 with order 2 or 3) and d_detections (2 K uint64); d_work holds image_work_bytes(K, P, max_pairs) bytes on a 16-byte boundary
        and its first uint64 receives the number of pairs found (more than max_pairs: nothing was deposited).  Stream-ordered: no
        allocation, no free, no wait."""
        check(lib.hare_image_device(self._h, self._kind, int(top_index), int(n_weight), capi.channel_flags(directional, order),
                                    int(n_bins), float(bin_len), int(frac_bits), int(max_pairs), d_work or None, d_hist or None,
                                    d_detections or None, stream or None))

    @staticmethod
    def image2_work_bytes(P: int, max_cands: int, max_paths: int) -> int:
        """Bytes of Image2_device's d_work for P polygons and lists of max_cands candidates and max_paths paths:
        HARE_IMAGE2_WORK_BYTES(P, max_cands, max_paths)."""
        return 256 + 32 * int(P) + 32 * int(max_cands) + 212 * int(max_paths)

    def Image2_device(self, n_weight: int, n_bins: int, bin_len: float, frac_bits: int, max_cands: int, max_paths: int, d_work: int, d_hist: int,
                      d_detections: int, top_index: int = 0, directional: bool = False, stream: int = 0, *, order: int = 1):
        """hare_image2_device on raw device addresses + a hipStream_t: the second-order image sources of the scene's source
        (include/hare_hip.h, "Image sources (second order)") -- the candidate stage polygons x polygons, the path stage receivers x
        candidates, three shadow rays per path and one deposit per path with all legs free, standing for n_weight source rays --
        accumulated into d_hist and d_detections (shaped as Image_device's); d_work holds image2_work_bytes(P, max_cands, max_paths) bytes on
        a 16-byte boundary and its first two uint64 receive the candidates and the paths found (either beyond its list: nothing was
        deposited).  Stream-ordered: no allocation, no free, no wait."""
        check(lib.hare_image2_device(self._h, self._kind, int(top_index), int(n_weight), capi.channel_flags(directional, order),
                                     int(n_bins), float(bin_len), int(frac_bits), int(max_cands), int(max_paths), d_work or None, d_hist or None,
                                     d_detections or None, stream or None))

    @staticmethod
    def diffract_work_bytes(K: int, max_pairs: int) -> int:
        """Bytes of diffract_device's d_work for K receivers and a list of max_pairs pairs: HARE_DIFFRACT_WORK_BYTES(K, max_pairs)."""
        return 256 + 68 * int(K) + 144 * int(max_pairs)

    def diffract_device(self, n_weight: int, n_bins: int, bin_len: float, frac_bits: int, max_pairs: int, d_work: int, d_hist: int,
                        d_detections: int, max_detour: float = float("inf"), top_index: int = 0, directional: bool = False, stream: int = 0, *,
                        order: int = 1):
        """hare_diffract_device on raw device addresses + a hipStream_t: first-order edge diffraction of the scene's source over the edges
        of set_edges (include/hare_hip.h, "Edge diffraction (first order)") -- the pair search edges x receivers, two shadow rays per
        accepted pair and one deposit per pair whose receiver the source does not see and whose legs are free, standing for n_weight
        source rays -- accumulated into d_hist and d_detections (shaped as direct_device's); d_work holds
        diffract_work_bytes(K, max_pairs) bytes on a 16-byte boundary and its first uint64 receives the number of pairs found (more than
        max_pairs: nothing was deposited).  Stream-ordered: no allocation, no free, no wait."""
        check(lib.hare_diffract_device(self._h, self._kind, int(top_index), int(n_weight), capi.channel_flags(directional, order),
                                       int(n_bins), float(bin_len), int(frac_bits), float(max_detour), int(max_pairs), d_work or None,
                                       d_hist or None, d_detections or None, stream or None))

    def Diffract_paths(self, n_weight: int, n_bins: int, bin_len: float, max_pairs: int, frac_bits: int = 40, max_detour: float = float("inf"),
                       top_index: int = 0, directional: bool = False, *, order: int = 1):
        """hare_diffract_paths: the same from the host, into a zeroed histogram.  Returns (hist uint64 [K, n_bins, B] or [K, n_bins, B, C],
        detections uint64 [K, 2], pairs found); a HareError with HARE_E_NOMEM, the count in its message and in its `found`, when the scene
        yields more than max_pairs pairs.  Add it to Source_paths' or a receive call's histogram as wrapping uint64 words."""
        shape = self._receive_shape(top_index, n_bins, bool(directional), order=order)
        K = max(shape[0], 0)
        hist, det, found = np.zeros((K,) + shape[1:], np.uint64), np.zeros((K, 2), np.uint64), np.zeros(1, np.uint64)
        try:
            check(lib.hare_diffract_paths(self._h, self._kind, int(top_index), int(n_weight), capi.channel_flags(directional, order), int(n_bins),
                                          float(bin_len), int(frac_bits), float(max_detour), int(max_pairs), ptr(hist), ptr(det), ptr(found)))
        except capi.HareError as e:
            e.found = int(found[0])
            raise
        return hist, det, int(found[0])

    @staticmethod
    def receive_work_bytes(n: int, rain: bool = False, image2: bool = False) -> int:
        """Bytes of receive_device's d_work for n rays: 2 n int32, or HARE_RECEIVE_RAIN_WORK_BYTES(n) with rain; with image2,
        HARE_RECEIVE_IMAGE2_WORK_BYTES(n) = n more behind either."""
        return (80 * int(n) + 256 if rain else 8 * int(n)) + (int(n) if image2 else 0)

    def receive_device(self, n: int, d_rays: int, bounces: int, n_bins: int, bin_len: float, frac_bits: int, d_state: int, d_work: int,
                       d_events_last: int, d_hist: int, d_detections: int, top_index: int = 0, d_excl1: int = 0, d_excl2: int = 0,
                       d_counters: int = 0, stream: int = 0, flags: int = 0, rain: bool = False, directional: bool = False,
                       time_limit: bool = False, direct: bool = False, image: bool = False, image2: bool = False, *, order: int = 1):
        """hare_receive_device on raw device addresses (e.g. torch.Tensor.data_ptr()) + a hipStream_t: d_state (1 + B) x n doubles is read
        and overwritten, d_hist (K x n_bins x B uint64) and d_detections (2 K uint64) are accumulated into.  Stream-ordered.  rain: diffuse
        rain (HARE_RECEIVE_DIFFUSE_RAIN); d_work then holds receive_work_bytes(n, rain=True) bytes.  directional
        (HARE_RECEIVE_DIRECTIONAL): d_hist is K x n_bins x B x 4 uint64, channels W, X, Y, Z (order 2, 3: x 9, x 16).  time_limit (HARE_RECEIVE_TIME_LIMIT): as
        in Receive_batch; a retired ray keeps the ray and the state of the cast that retired it.  direct (HARE_RECEIVE_DIRECT): cast 0
        detects nothing -- the rays are the scene's source's, and direct_device deposits their direct sound."""
        if direct:
            flags |= capi.RECEIVE_DIRECT
        if image:                                    # suppression only ("Image sources (first order)"): Image_device makes the deposit
            flags |= capi.RECEIVE_IMAGE
        if image2:                                   # suppression only ("Image sources (second order)"): Image2_device makes the deposit;
            flags |= capi.RECEIVE_IMAGE2             # d_work then holds receive_work_bytes(n, rain, image2=True) bytes
        if time_limit:
            flags |= capi.RECEIVE_TIME_LIMIT
        if rain:
            flags |= capi.RECEIVE_DIFFUSE_RAIN
        flags |= capi.channel_flags(directional, order)
        check(lib.hare_receive_device(self._h, self._kind, int(top_index), int(n), d_rays or None, d_excl1 or None, d_excl2 or None,
                                      int(bounces), int(flags), int(n_bins), float(bin_len), int(frac_bits), d_state or None, d_work or None,
                                      d_events_last or None, d_hist or None, d_detections or None, d_counters or None, stream or None))

    def shoot_device(self, n: int, d_rays: int, d_out: int, top_index: int = 0, d_excl1: int = 0, d_excl2: int = 0,
                     d_counters: int = 0, stream: int = 0, flags: int = 0):
        """Device-resident shoot: raw device addresses (e.g. torch.Tensor.data_ptr()) + a hipStream_t."""
        check(lib.hare_shoot_device(self._h, self._kind, int(top_index), int(n), d_rays or None, d_excl1 or None,
                                    d_excl2 or None, int(flags), d_out or None, d_counters or None, stream or None))

    def kernel_name(self, n: int, top_index: int = 0, flags: int = 0) -> str:
        """The gfx950 kernel a shoot of n rays launches (what rocprofv3 will list)."""
        return (lib.hare_shoot_kernel_name(self._h, self._kind, int(top_index), int(n), int(flags)) or b"").decode()

    def bounce_kernel_name(self, n: int, bounces: int, top_index: int = 0) -> str:
        """The fused kernel hare_bounce_device launches for n rays, or "" when it runs a launch per cast."""
        if bounces > 16:
            return ""
        name = self.kernel_name(n, top_index, flags=32)          # HARE_SHOOT_BOUNCE_LOOP
        return name if "bounce" in name else ""

    def reflect_device(self, n: int, d_rays: int, d_events: int, d_excl_out: int, top_index: int = 0, stream: int = 0):
        check(lib.hare_reflect_device(self._h, int(top_index), int(n), d_rays, d_events, d_excl_out, stream or None))

    def bounce_device(self, n: int, d_rays: int, bounces: int, d_work: int, d_events_last: int = 0, d_events_all: int = 0,
                      top_index: int = 0, d_excl1: int = 0, d_excl2: int = 0, d_counters: int = 0, d_counters_per_cast: int = 0,
                      stream: int = 0, flags: int = 0):
        """The bounce loop on device buffers (hare_bounce_device): `bounces` casts per ray, reflection + exclusion of the polygon left
        between them; d_rays is read and overwritten, d_work is 2 n int32 of scratch.  One launch for a Voxel_Grid where the pool
        kernel serves, else a launch per cast; stream-ordered, no host synchronisation."""
        check(lib.hare_bounce_device(self._h, self._kind, int(top_index), int(n), d_rays or None, d_excl1 or None, d_excl2 or None,
                                     int(bounces), int(flags), d_work or None, d_events_all or None, d_events_last or None,
                                     d_counters or None, d_counters_per_cast or None, stream or None))


class Voxel_Grid(Spatial_Partition):
    """Voxel_Grid(Topology[] Model_in, int Domain) / (Topology[] Model_in, int MaxDomain, int Avg_polys)
    (Voxel_Grid.cs:48, :128)."""

    _kind = KIND_VOXEL

    def __init__(self, Model_in, Domain: int, Avg_polys: Optional[int] = None, device: int = 0):
        super().__init__(Model_in, device)
        if Avg_polys is None:
            check(lib.hare_voxel_build(self._h, int(Domain)))
        else:
            check(lib.hare_voxel_build_adaptive(self._h, int(Domain), int(Avg_polys)))
        info = self.info()
        self.Char_Step = info.char_step
        self.VoxelCt = info.ct

    def info(self) -> capi.VoxelInfo:
        i = capi.VoxelInfo()
        check(lib.hare_voxel_get_info(self._h, C.addressof(i)))
        return i

    # public members of the reference class
    @property
    def Xdim(self):
        return self.info().box_dims[0]

    @property
    def Ydim(self):
        return self.info().box_dims[1]

    @property
    def Zdim(self):
        return self.info().box_dims[2]

    @property
    def MinPt(self):
        return tuple(self.info().obox_min)

    def PointInVoxel(self, Pt):
        """Voxel_Grid.PointInVoxel(Point, out X, out Y, out Z) (Voxel_Grid.cs:322-327)."""
        i = self.info()
        return tuple(int(np.floor((Pt[a] - i.obox_min[a]) / i.voxel_dims[a])) for a in range(3))

    def PointInVoxel_code(self, Pt) -> int:
        """int Voxel_Grid.PointInVoxel(Point) (Voxel_Grid.cs:329-332): the VoxelCode of the voxel holding Pt."""
        return self.VoxelCode(*self.PointInVoxel(Pt))

    def VoxelDecode(self, Code: int):
        """Voxel_Grid.VoxelDecode (Voxel_Grid.cs:256-262) -> (X, Y, Z)."""
        ct = self.VoxelCt
        Z = Code // (ct * ct)
        Code -= Z * ct * ct
        Y = Code // ct
        return Code - Y * ct, Y, Z

    def VoxelCode(self, X: int, Y: int, Z: int) -> int:
        """Voxel_Grid.VoxelCode (Voxel_Grid.cs:264-267): XYTot * Z + VoxelCtY * X + Y."""
        ct = self.VoxelCt
        return ct * ct * Z + ct * X + Y

    def Voxel_Inv(self, top_index: int = 0):
        """Voxel_Inv[x,y,z,top] as CSR (cell = (x*ct + y)*ct + z)."""
        i = self.info()
        n = i.ct ** 3
        start = np.zeros(n + 1, np.uint32)
        check(lib.hare_voxel_get_lists(self._h, int(top_index), ptr(start), None))
        items = np.zeros(max(1, int(start[-1])), np.int32)
        check(lib.hare_voxel_get_lists(self._h, int(top_index), ptr(start), ptr(items)))
        return start, items[: int(start[-1])]


class Octree(Spatial_Partition):
    """Octree(Topology[] Model_In, int maxDepth, int maxPolygonsPerNode) ("Octree - alt.cs":45)."""

    _kind = KIND_OCTREE

    def __init__(self, Model_In, maxDepth: int, maxPolygonsPerNode: int, device: int = 0):
        super().__init__(Model_In, device)
        check(lib.hare_octree_build(self._h, int(maxDepth), int(maxPolygonsPerNode)))

    def info(self) -> capi.TreeInfo:
        i = capi.TreeInfo()
        check(lib.hare_octree_get_info(self._h, C.addressof(i)))
        return i

    def nodes(self):
        i = self.info()
        n, tot = i.n_nodes, int(i.total_items)
        boxes = np.zeros((n, 6))
        fc = np.zeros(n, np.int32)
        st = np.zeros(n, np.int32)
        cn = np.zeros(n, np.int32)
        items = np.zeros(max(tot, 1), np.int32)
        check(lib.hare_octree_get_nodes(self._h, ptr(boxes), ptr(fc), ptr(st), ptr(cn), ptr(items)))
        return boxes, fc, st, cn, items[:tot]


class KDTree(Spatial_Partition):
    """KDTree(Topology[] Model_In, int maxDepth, int maxPolygonsPerNode) (KDTree.cs:51)."""

    _kind = KIND_KDTREE

    def __init__(self, Model_In, maxDepth: int, maxPolygonsPerNode: int, device: int = 0):
        super().__init__(Model_In, device)
        check(lib.hare_kdtree_build(self._h, int(maxDepth), int(maxPolygonsPerNode)))

    def info(self) -> capi.TreeInfo:
        i = capi.TreeInfo()
        check(lib.hare_kdtree_get_info(self._h, C.addressof(i)))
        return i

    def nodes(self):
        i = self.info()
        n, tot = i.n_nodes, int(i.total_items)
        boxes = np.zeros((n, 6))
        split = np.zeros(n)
        axis = np.zeros(n, np.int32)
        left = np.zeros(n, np.int32)
        right = np.zeros(n, np.int32)
        st = np.zeros(n, np.int32)
        cn = np.zeros(n, np.int32)
        items = np.zeros(max(tot, 1), np.int32)
        check(lib.hare_kdtree_get_nodes(self._h, ptr(boxes), ptr(split), ptr(axis), ptr(left), ptr(right), ptr(st),
                                        ptr(cn), ptr(items)))
        return boxes, split, axis, left, right, st, cn, items[:tot]
