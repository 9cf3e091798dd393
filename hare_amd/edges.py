"""Host-side helpers for first-order edge diffraction (include/hare_hip.h, "receivers", "Edge diffraction (first order)").  The contract
does no edge detection: hare_scene_set_edges takes the caller's edges.  find_edges proposes them from a topology and band_inv_lambda forms
the setter's f_b / c; both are plain numpy on the host and no part of the contract -- a caller with better knowledge of the model (a CAD
layer of barrier tops, say) passes its own."""
import numpy as np


def _mesh(topology):
    if hasattr(topology, "verts") and hasattr(topology, "nverts"):
        return np.asarray(topology.verts, np.float64), np.asarray(topology.nverts, np.int32)
    verts, nverts = topology
    return np.asarray(verts, np.float64), np.asarray(nverts, np.int32)


def _crossings(o, d, tris):
    """How many of the triangles [T, 3, 3] the ray o + s d, s > 0, passes through (Moeller-Trumbore, edges not counted twice with care: the
    caller retries another direction when the two sides of a face do not differ by one)."""
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    pv = np.cross(d[None], e2)
    det = (e1 * pv).sum(axis=1)
    ok = np.abs(det) > 1e-300
    inv = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
    tv = o[None] - tris[:, 0]
    u = (tv * pv).sum(axis=1) * inv
    qv = np.cross(tv, e1)
    v = (qv * d[None]).sum(axis=1) * inv
    s = (e2 * qv).sum(axis=1) * inv
    return int((ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (s > 0)).sum())


def find_edges(topology, min_angle_deg: float = 10.0, enclosed: bool = True):
    """The diffracting edges of a topology (a hare_amd.Topology, or (verts [P, 4, 3], nverts [P])): returns (ends float64 [E, 2, 3], faces
    int32 [E, 2]) for Spatial_Partition.set_edges.
      - An edge that two polygons share (the same two corners, bit for bit) is returned with both faces when the air-side dihedral opens
        by more than min_angle_deg beyond flat: the wedge of solid is convex and its faces' normals differ by more than that.  The corners
        of a room seen from inside are concave and the diagonal of a split quadrilateral is flat: neither is returned.  The polygons'
        winding is not trusted: every closed surface (a connected set of polygons without a free edge) is oriented from one of its faces by
        the winding across shared edges, and the air side of that face is found by counting how many closed surfaces a ray from it crosses.
        enclosed=True (a room: the outermost closed surface holds the air) takes the odd side as air; enclosed=False (obstacles in the
        open) the even side.
      - An edge of one polygon only (a free edge of a screen) is returned with faces (p, -1), whatever the angle.
      - An edge that more than two polygons share is skipped, and so is a T-junction (corners that do not coincide): pass such edges
        yourself."""
    verts, nverts = _mesh(topology)
    P = verts.shape[0]
    e1, e2 = verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]
    normals = np.cross(e1, e2)
    area2 = np.sqrt((normals * normals).sum(axis=1))
    normals = normals / np.where(area2 > 0, area2, 1.0)[:, None]
    table = {}
    for p in range(P):
        nv = int(nverts[p])
        for i in range(nv):
            a, b = verts[p, i], verts[p, (i + 1) % nv]
            ka, kb = a.tobytes(), b.tobytes()
            if ka != kb:
                table.setdefault((ka, kb) if ka < kb else (kb, ka), []).append((p, ka))
    # ---- the surfaces: polygons joined across the edges that exactly two of them share; one with a free or crowded edge is open
    parent = list(range(P))

    def root(p):
        while parent[p] != p:
            parent[p] = parent[parent[p]]
            p = parent[p]
        return p
    shared, free = [], []
    for key, users in table.items():
        if len(users) == 2:
            (p, ka), (q, kq) = users
            if p != q:
                shared.append((p, q, ka == kq, key))
                parent[root(p)] = root(q)
        elif len(users) == 1:
            free.append((users[0][0], key))
    is_open = np.zeros(P, bool)
    for key, users in table.items():
        if len(users) != 2 or users[0][0] == users[1][0]:
            for p, _ in users:
                is_open[root(p)] = True
    comp = np.array([root(p) for p in range(P)])
    closed = ~is_open[comp]
    # ---- each closed surface oriented from its largest face: sign[p] = +1 where p's normal points to the same side as that face's
    sign = np.zeros(P)
    nbrs = {}
    for p, q, same_dir, _ in shared:
        nbrs.setdefault(p, []).append((q, same_dir))
        nbrs.setdefault(q, []).append((p, same_dir))
    tri = np.concatenate([verts[closed][:, [0, 1, 2]], verts[closed & (nverts == 4)][:, [0, 2, 3]]]) if closed.any() else np.zeros((0, 3, 3))
    scale = float(np.abs(verts).max()) + 1.0
    for c in np.unique(comp[closed]):
        members = np.nonzero(comp == c)[0]
        start = int(members[np.argmax(area2[members])])
        sign[start] = 1.0
        stack = [start]
        while stack:
            p = stack.pop()
            for q, same_dir in nbrs.get(p, ()):
                if sign[q] == 0:
                    sign[q] = -sign[p] if same_dir else sign[p]      # consistent windings run a shared edge in opposite directions
                    stack.append(q)
        mid = verts[start, :3].mean(axis=0)
        air = 1.0
        for d in ((0.5377, 0.6613, 0.5231), (-0.3119, 0.7723, 0.5533), (0.8013, -0.1237, 0.5853), (0.2311, 0.4127, -0.8811)):
            d = np.asarray(d)
            up = _crossings(mid + normals[start] * (1e-7 * scale), d, tri)
            down = _crossings(mid - normals[start] * (1e-7 * scale), d, tri)
            if abs(up - down) == 1:
                air = 1.0 if (up % 2 == 1) == bool(enclosed) else -1.0
                break
        sign[members] *= air
    ends, faces = [], []
    cos_min = np.cos(np.radians(float(min_angle_deg)))
    for p, key in free:
        ends.append((np.frombuffer(key[0]), np.frombuffer(key[1])))
        faces.append((p, -1))
    for p, q, _, key in shared:
        if not closed[p] or sign[p] == 0 or sign[q] == 0:
            continue
        a = np.frombuffer(key[0])
        np_air, nq_air = normals[p] * sign[p], normals[q] * sign[q]
        mid_q = verts[q, :int(nverts[q])].mean(axis=0)
        if np_air @ (mid_q - a) < 0 and np_air @ nq_air < cos_min:      # q falls away behind p's air side, and by more than the threshold
            ends.append((a, np.frombuffer(key[1])))
            faces.append((min(p, q), max(p, q)))
    return (np.array(ends, np.float64).reshape(-1, 2, 3), np.array(faces, np.int32).reshape(-1, 2))


def band_inv_lambda(freqs, c: float = 343.0):
    """f_b / c per band in 1/m, the setter's inv_lambda: freqs in Hz (the bands' centre frequencies), c the speed of sound in m/s."""
    f = np.asarray(freqs, np.float64).reshape(-1)
    if not (np.isfinite(f).all() and (f >= 0).all() and np.isfinite(c) and c > 0):
        raise ValueError("frequencies must be finite and >= 0, c finite and > 0")
    return f / np.float64(c)
