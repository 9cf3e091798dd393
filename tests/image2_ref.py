"""numpy restatement of the second-order image sources (include/hare_hip.h, "receivers", "Image sources (second order)"): the source
mirrored in every polygon's plane, that image mirrored again in every other polygon's plane, the brute-force search receivers x polygons x
polygons with the reference's two-sided polygon test at q and at p, three shadow rays per accepted path and one deposit per path with all
legs free -- operation for operation in FP64.  Written on tests/image_ref.py (mirror, tri_fast, the scenes and oracles), tests/receive_ref.py
(deposit, receive_loop) and the oracle partition's shoot for the legs.  hare_image2_device's histogram and detections must match image2()
byte for byte.  suppressed2() restates the flag's suppression rule on top of tests/receive_ref.py's loop.  cases() are the device cases of
tests/test_gpu_image2.py; tests/test_image2_ref.py asserts on the CPU that they hold what they claim to hold."""
import dataclasses

import numpy as np

from oracle import pyoracle as po
from tests import image_ref as ir
from tests.direct_ref import share
from tests.image_ref import dot3, mesh_of, oracle_of, tri_fast
from tests.receive_ref import deposit, receive_loop
from tests.scatter_ref import choose, ray_base, uniform, weights
from tests.source_ref import lookup


def poly_fast_rows(o, d, verts, nverts, normals):
    """hare_math.h's poly_fast row by row: rays o, d [N, 3] against their own polygons verts [N, 4, 3], nverts [N], normals [N, 3]."""
    with np.errstate(all="ignore"):
        side = ~(dot3(d[:, 0], d[:, 1], d[:, 2], normals[:, 0], normals[:, 1], normals[:, 2]) < 0)
    quad = nverts == 4
    v0, v1, v2, v3 = (verts[:, i, :] for i in range(4))
    ha, ta = tri_fast(o, d, v0, v1, v2)
    hb, tb = tri_fast(o, d, v2, v3, v0)
    hc, tc = tri_fast(o, d, v2, v1, v0)
    hd, td = tri_fast(o, d, v0, v3, v2)
    hit_front, t_front = ha | (quad & hb), np.where(ha, ta, np.where(quad & hb, tb, 0.0))
    hit_back, t_back = hc | (quad & hd), np.where(hc, tc, np.where(quad & hd, td, 0.0))
    return np.where(side, hit_front, hit_back), np.where(side, t_front, t_back)


def candidates(pos, verts, normals):
    """Every ordered pair (p, q) with mirrored2: dict of p, q [C], S1 [P, 3], S2 [C, 3], and the classes `h2_zero` (pairs p != q with
    mirrored_p, nn_q > 0 and h2 == 0), `same` (the pairs p == q skipped for a mirrored p), `unmirrored` [P]."""
    S1, mir1, _ = ir.mirror(pos, verts, normals)
    P = verts.shape[0]
    v0 = verts[:, 0, :]
    n = normals
    with np.errstate(all="ignore"):
        h2 = dot3(S1[:, None, 0] - v0[None, :, 0], S1[:, None, 1] - v0[None, :, 1], S1[:, None, 2] - v0[None, :, 2], n[None, :, 0], n[None, :, 1],
                  n[None, :, 2])                                                            # [p, q]
        nn = dot3(n[:, 0], n[:, 1], n[:, 2], n[:, 0], n[:, 1], n[:, 2])
        base = mir1[:, None] & (nn > 0)[None, :] & ~np.eye(P, dtype=bool)
        mir2 = base & ((h2 > 0) | (h2 < 0))
        p, q = np.nonzero(mir2)
        k2 = (2.0 * h2[p, q]) / nn[q]
        S2 = np.stack([S1[p, 0] - n[q, 0] * k2, S1[p, 1] - n[q, 1] * k2, S1[p, 2] - n[q, 2] * k2], axis=1)
    return dict(p=p, q=q, S1=S1, S2=S2, h2_zero=int((base & (h2 == 0)).sum()), same=int(mir1.sum()), unmirrored=~mir1)


def paths(pos, verts, nverts, normals, centers, radii, chunk=1 << 20):
    """The brute-force search over K x P x P: dict of k, p, q [m] (the accepted paths), x1, x2, v [m, 3], d2 [m], the candidates() dict as
    `cands`, and `ineligible` (triples with on_q && on_p and d2 <= rr)."""
    centers = np.asarray(centers, np.float64).reshape(-1, 3)
    rr = np.asarray(radii, np.float64) * np.asarray(radii, np.float64)
    c = candidates(pos, verts, normals)
    cp, cq, S1, S2 = c["p"], c["q"], c["S1"], c["S2"]
    out = {k: [] for k in ("k", "p", "q", "x1", "x2", "v", "d2")}
    ineligible = 0
    for k in range(centers.shape[0]):
        for lo in range(0, cp.size, chunk):
            p, q, s2 = cp[lo:lo + chunk], cq[lo:lo + chunk], S2[lo:lo + chunk]
            v = centers[k][None] - s2
            d2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
            hit, t2 = poly_fast_rows(s2, v, verts[q], nverts[q], normals[q])
            i = np.nonzero(hit & (t2 > 0.0) & (t2 < 1.0))[0]                               # on_q
            if not i.size:
                continue
            tt = t2[i]
            x2 = np.stack([s2[i, 0] + v[i, 0] * tt, s2[i, 1] + v[i, 1] * tt, s2[i, 2] + v[i, 2] * tt], axis=1)
            s1 = S1[p[i]]
            w = x2 - s1
            hit, t1 = poly_fast_rows(s1, w, verts[p[i]], nverts[p[i]], normals[p[i]])
            j = np.nonzero(hit & (t1 > 0.0) & (t1 < 1.0))[0]                               # on_p
            elig = d2[i[j]] > rr[k]
            ineligible += int((~elig).sum())
            j = j[elig]
            if not j.size:
                continue
            tt = t1[j]
            x1 = np.stack([s1[j, 0] + w[j, 0] * tt, s1[j, 1] + w[j, 1] * tt, s1[j, 2] + w[j, 2] * tt], axis=1)
            for name, val in (("k", np.full(j.size, k)), ("p", p[i[j]]), ("q", q[i[j]]), ("x1", x1), ("x2", x2[j]), ("v", v[i[j]]), ("d2", d2[i[j]])):
                out[name].append(val)
    cat = lambda name, shape: np.concatenate(out[name]) if out[name] else np.zeros(shape, np.int64 if name in "kpq" else np.float64)
    res = {name: cat(name, (0, 3) if name in ("x1", "x2", "v") else (0,)) for name in out}
    res.update(cands=c, ineligible=ineligible)
    return res


def image2(part, verts, nverts, normals, pos, power, frame, R, gain, alpha, sigma, centers, radii, n_weight, n_bins, bin_len, frac_bits, hist, det,
           seen=None, tallies=None, nthreads=16):
    """The second-order image sources, accumulated into hist and det as tests/image_ref.py's image() does for the first order (same
    arguments).  Returns (candidates, paths) found.  seen (dict, optional) receives paths()'s dict and, per path, occ (three columns:
    x2 -> center, x1 -> x2, x1 -> source), binned, edge."""
    pos = np.asarray(pos, np.float64).reshape(3)
    power = np.asarray(power, np.float64).reshape(-1)
    centers = np.asarray(centers, np.float64).reshape(-1, 3)
    rr = np.asarray(radii, np.float64) * np.asarray(radii, np.float64)
    B = power.shape[0]
    W = np.float64(int(n_weight))
    f = paths(pos, verts, nverts, normals, centers, radii)
    k, p, q, x1, x2 = f["k"], f["p"], f["q"], f["x1"], f["x2"]
    m = k.size
    occ = np.zeros((m, 3), bool)
    if m:
        p32, q32, none = p.astype(np.int32), q.astype(np.int32), np.full(m, -1, np.int32)
        legs = ((x2, centers[k] - x2, q32, none), (x1, x2 - x1, p32, q32), (x1, pos[None] - x1, p32, none))
        for col, (o, d, e1, e2) in enumerate(legs):
            ev, _ = part.shoot(np.ascontiguousarray(np.concatenate([o, d], axis=1)), excl1=e1, excl2=e2, nthreads=nthreads)
            occ[:, col] = (ev["hit"] == 1) & (ev["t"] < 1.0)
    free = np.nonzero(~occ.any(axis=1))[0]
    d2 = f["d2"][free]
    dist = np.sqrt(d2)
    fw = share(rr[k[free]], d2) * W
    g = np.ones((free.size, B))
    if R and free.size:
        F, iv, iu, _ = lookup(x1[free] - pos[None], np.eye(3) if frame is None else frame, R)
        g = np.asarray(gain, np.float64).reshape(6, R, R, -1)[F, iv, iu, :]
    P = verts.shape[0]
    al = np.zeros((P, B)) if alpha is None else np.asarray(alpha, np.float64)
    sg = np.zeros((P, B)) if sigma is None else np.asarray(sigma, np.float64)
    r = ((1.0 - al[p[free]]) * (1.0 - sg[p[free]])) * ((1.0 - al[q[free]]) * (1.0 - sg[q[free]]))
    xb = dist / np.float64(bin_len)
    binned = (xb >= 0) & (xb < np.float64(n_bins))
    np.add.at(det[:, 0], k[free][binned], np.uint64(1))
    np.add.at(det[:, 1], k[free][~binned], np.uint64(1))
    for j in np.nonzero(binned)[0]:
        val = (((power * g[j]) * r[j]) * fw[j])[:, None]
        vj = f["v"][free[j]]

        def arrival():
            return -(vj[0:1] / dist[j]), -(vj[1:2] / dist[j]), -(vj[2:3] / dist[j])
        deposit(hist, int(k[free[j]]), np.array([int(np.floor(xb[j]))]), val, frac_bits, arrival, None, tallies)
    if seen is not None:
        full = np.zeros(m, bool)
        full[free] = binned
        edge = np.zeros(m, bool)
        edge[free] = xb == np.floor(xb)
        seen.update(f, occ=occ, binned=full, edge=edge)
    return f["cands"]["p"].size, m


def suppressed2(topo, part, rays, state_in, bounces, centers, radii, n_bins, bin_len, frac_bits, alpha=None, sigma=None, seed=0, g0=0, rain=False,
                directional=False, visit=None, nthreads=16):
    """The receive loop of a call with HARE_RECEIVE_IMAGE | HARE_RECEIVE_IMAGE2 and no termination rule, WITHOUT the deposits:
    tests/image_ref.py's suppressed() minus cast 2's receiver step over the rays whose reflections behind cast 0 and behind cast 1 were both
    specular -- every ray that hit twice when there is no table, the rays with !(u < p) at c = 0 and at c = 1 when there is one.  That step
    is the loop itself, run for one cast on those rays as they leave cast 1.  Returns (hist, det, state, dict(twice: ray count, other: rays
    alive in cast 2 that are not suppressed))."""
    kw = dict(alpha=alpha, sigma=sigma, seed=seed, rain=rain, directional=directional, visit=visit, nthreads=nthreads)
    hist, det, state, _ = ir.suppressed(topo, part, rays, state_in, bounces, centers, radii, n_bins, bin_len, frac_bits, g0=g0, **kw)
    if bounces < 3:
        return hist, det, state, dict(twice=0, other=0)
    n = rays.shape[0]
    last = []
    _, _, st2, kept = receive_loop(po, topo, part, rays, 3, centers, radii, n_bins, bin_len, frac_bits, state_in=state_in, g0=g0, keep_rays_after=1, **kw)
    _, _, st, _ = receive_loop(po, topo, part, rays, 2, centers, radii, n_bins, bin_len, frac_bits, state_in=state_in, g0=g0, last_events=last, **kw)
    ev0 = part.shoot(np.ascontiguousarray(rays), nthreads=nthreads)[0]
    ev1 = last[0]
    alive = (ev0["hit"] == 1) & (ev1["hit"] == 1)                   # the rays of cast 2
    idx = np.nonzero(alive)[0]
    L, E = st[0, idx], st[1:, idx].copy()                           # behind cast 1's update, before its choice's weights
    spec = np.ones(idx.size, bool)
    if sigma is not None:
        sg = np.asarray(sigma, np.float64)
        base = ray_base(seed, np.arange(g0, g0 + n, dtype=np.uint64))
        _, d0 = choose(sg[ev0["poly_id"][idx]], uniform(base[idx], 0, 0))
        row1 = sg[ev1["poly_id"][idx]]
        p1, d1 = choose(row1, uniform(base[idx], 1, 0))
        E = E * weights(row1, p1, d1).T
        spec = ~d0 & ~d1
    sp = idx[spec]
    if sp.size:
        h1, dd, _, _ = receive_loop(po, topo, part, kept[sp], 1, centers, radii, n_bins, bin_len, frac_bits,
                                    state_in=np.concatenate([L[None, spec], E[:, spec]], axis=0), excl1=ev1["poly_id"][sp], directional=directional,
                                    visit=visit, nthreads=nthreads, alpha=alpha)
        with np.errstate(over="ignore"):
            hist, det = hist - h1, det - dd
    return hist, det, state, dict(twice=int(sp.size), other=int(idx.size - sp.size))


# ---- the device cases (tests/test_gpu_image2.py), on tests/image_ref.py's scenes
PLACED = dict(ir.PLACED)
# the 12-triangle shoebox with the source at (3, 2, 1): receiver 0 is reached off the floor and the ceiling (z: 1 -> 0 -> 4 -> 1, 8 m on the
# z axis alone) through both walls' diagonals; receiver 1 at 10 m of path via the walls x = 0 and x = 10
PLACED["box12"] = [((7.0, 5.0, 1.0), 0.25, "paths through the diagonals the floor's and the ceiling's triangles share"),
                   ((7.0, 2.0, 1.0), 0.25, "x: 3 -> 0 -> 10 -> 7 is 16 m; via x = 10 then x = 0: 3 -> 10 -> 0 -> 7, 24 m: on bin edges"),
                   ((3.0, 0.25, 1.0), 2.5, "second images inside the sphere: not eligible")]


# "corner3": three mutually perpendicular triangles that share the corner (1, 1, 1), where the source of its case sits: the source lies in the
# plane of every polygon (h == 0 three times), so no polygon has an image and there is NO candidate at all -- not among tests/image_ref.py's
# scenes, which are closed rooms and always mirror the source somewhere.  Registered with image_ref's meshes so that its helpers serve it
CORNER = (1.0, 1.0, 1.0)
_c3 = np.zeros((3, 4, 3))
_c3[0, :3] = [CORNER, (3.0, 1.0, 1.0), (1.0, 3.0, 1.0)]            # in z = 1
_c3[1, :3] = [CORNER, (1.0, 3.0, 1.0), (1.0, 1.0, 3.0)]            # in x = 1
_c3[2, :3] = [CORNER, (1.0, 1.0, 3.0), (3.0, 1.0, 1.0)]            # in y = 1
ir._MESHES.setdefault("corner3", (_c3, np.full(3, 3, np.int32), (3.0, 3.0, 3.0)))
PLACED["corner3"] = [((2.0, 2.0, 2.0), 0.25, "in front of all three triangles")]


@dataclasses.dataclass
class Image2Case(ir.ImageCase):
    def receivers(self):
        rng = np.random.default_rng(91 + self.K)
        _, _, size = mesh_of(self.scene)
        c = rng.uniform(0.08, 0.92, (self.K, 3)) * np.asarray(size)
        r = rng.uniform(0.1, 0.3, self.K)
        for k, (ck, rk, _) in enumerate(PLACED[self.scene][:self.K]):
            c[k], r[k] = ck, rk
        if self.big:
            r[0] = 100.0
        return np.ascontiguousarray(c), r


def cases():
    """Four scenes of tests/test_gpu_image.py (P = 12, 54, 56, 972) and the three-triangle corner without a candidate; every partition; K = 1, 8, 256 linear and 257 as a map (K <= 8 at P = 972: the brute force is
    K x P x P); B = 1, 3, 8; with and without a directivity table; absorption alone and with scattering; one and four channels."""
    C = Image2Case
    V, O, T = ir.PARTITIONS
    out = [C("box12-K1", "box12", V, 1, False, 1, 0, "none", 40, 64, 0.5, False, 4097),
           C("box12-K8-dir", "box12", O, 8, False, 3, 4, "alpha", 0, 32, 0.5, True, 1),
           C("box12-K1-none", "box12", T, 1, False, 1, 0, "alpha", 40, 8, 1.0, False, 4097, big=True),
           C("box12-K256", "box12", T, 256, False, 8, 0, "alpha+sigma", 62, 64, 0.25, False, 2 ** 40),
           C("box972-K1", "box972", O, 1, False, 3, 4, "alpha+sigma", 40, 64, 0.25, False, 4097),
           C("box972-K8-dir", "box972", V, 8, False, 3, 0, "alpha", 40, 256, 2.0 ** -3, True, 4097),
           C("quads-K8", "quads", V, 8, False, 1, 4, "alpha+sigma", 40, 48, 0.5, False, 2 ** 40),
           C("quads-map257-dir", "quads", O, 257, True, 3, 0, "alpha", 40, 32, 1.0, True, 1),
           C("quads-K256", "quads", T, 256, False, 8, 0, "alpha", 40, 1, 64.0, False, 4097),
           C("baffle-K8", "baffle", V, 8, False, 3, 4, "alpha+sigma", 40, 64, 0.5, False, 4097, pos=(2.0, 1.0, 1.0)),
           C("baffle-K256-dir", "baffle", O, 256, False, 1, 0, "alpha", 40, 32, 1.0, True, 4097, pos=(2.0, 1.0, 1.0)),
           C("baffle-map257-h0", "baffle", T, 257, True, 3, 0, "alpha", 40, 64, 0.5, False, 1, pos=(5.0, 3.5, 1.0)),
           C("corner3-K8-nocands", "corner3", V, 8, False, 3, 0, "alpha", 40, 16, 0.5, False, 4097, pos=CORNER)]
    assert len({c.name for c in out}) == len(out)
    return out


_KEPT = {}


def reference(case, nthreads=16):
    """image2() of a case onto zeros: dict of hist, det, cands, paths, seen and tallies.  Kept and served again."""
    if case.name in _KEPT:
        return _KEPT[case.name]
    verts, nverts, _ = mesh_of(case.scene)
    _, o, normals = oracle_of(case.scene, case.partition)
    hist = np.zeros(case.shape, np.uint64)
    det = np.zeros((case.K, 2), np.uint64)
    centers, radii = case.receivers()
    alpha, sigma = case.absorption()
    seen, tallies = {}, {}
    nc, m = image2(o, verts, nverts, normals, *case.source(), alpha, sigma, centers, radii, case.n_weight, case.n_bins, case.bin_len,
                   case.frac_bits, hist, det, seen, tallies, nthreads)
    out = _KEPT[case.name] = dict(hist=hist, det=det, cands=nc, paths=m, seen=seen, tallies=tallies)
    return out
