"""numpy restatement of first-order edge diffraction (include/hare_hip.h, "receivers", "Edge diffraction (first order)"): the direct shadow
ray per receiver, the pair search edges x receivers for the apex of the shortest path over each edge, two shadow rays per accepted pair
with both faces of the edge excluded, and one deposit per pair whose receiver the source does not see and whose legs are free, attenuated
by 1 / (3 + 20 N) -- operation for operation in FP64.  Written on what exists: the shadow rays are answered by the oracle partition's shoot
as tests/image_ref.py answers its own, and the deposit is that module's (share, lookup, deposit: read through the module, so
tests/ambi_ref.py's higher orders apply to it).  hare_diffract_device's histogram, detections and pair count must match diffract() byte
for byte."""
import numpy as np

from tests import image_ref as ir
from tests.direct_ref import share
from tests.image_ref import dot3
from tests.source_ref import lookup


def _dot(x, y):
    return dot3(x[..., 0], x[..., 1], x[..., 2], y[..., 0], y[..., 1], y[..., 2])


def pairs(pos, ends, centers, radii, max_detour):
    """The pair search: dict of j, k [m] (the accepted pairs), A, u, w [m, 3], ls, lr, delta [m], eligible [K], d2 [K], and the classes the
    search went through as counts over the pairs with an eligible receiver -- t0, t1 (the apex exactly at an end), on_line (hsum == 0),
    in_sphere (the apex inside the receiver's sphere), at_limit (delta == max_detour), over_limit (delta > max_detour)."""
    S = np.asarray(pos, np.float64).reshape(3)
    ends = np.asarray(ends, np.float64).reshape(-1, 2, 3)
    c = np.asarray(centers, np.float64).reshape(-1, 3)
    rr = np.asarray(radii, np.float64) * np.asarray(radii, np.float64)
    md = np.float64(max_detour)
    with np.errstate(all="ignore"):
        v = c - S[None]
        d2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        elig = d2 > rr
        a = ends[:, 0]
        e = ends[:, 1] - ends[:, 0]                                                 # [E, 3]
        ee = _dot(e, e)
        ts = _dot(S[None] - a, e) / ee
        ps = S[None] - (a + e * ts[:, None])
        hs = np.sqrt(_dot(ps, ps))                                                  # [E]
        A_, E_ = a[:, None, :], e[:, None, :]                                       # [E, 1, 3]
        C_ = c[None, :, :]
        tr = _dot(C_ - A_, E_) / ee[:, None]                                        # [E, K]
        pr = C_ - (A_ + E_ * tr[..., None])
        hr = np.sqrt(_dot(pr, pr))
        hsum = hs[:, None] + hr
        t = (ts[:, None] * hr + tr * hs[:, None]) / hsum
        A = A_ + E_ * t[..., None]
        u = A - S[None, None]
        w = C_ - A
        ls2, lr2 = _dot(u, u), _dot(w, w)
        ls, lr = np.sqrt(ls2), np.sqrt(lr2)
        delta = (ls + lr) - np.sqrt(d2)[None, :]
        inside = (hsum > 0) & (t > 0) & (t < 1) & (ls2 > 0)
        acc = elig[None] & inside & (lr2 > rr[None]) & (delta > 0) & (delta <= md)
        el = np.broadcast_to(elig[None], acc.shape)
        classes = dict(t0=int((el & (t == 0)).sum()), t1=int((el & (t == 1)).sum()), on_line=int((el & (hsum == 0)).sum()),
                       in_sphere=int((el & inside & ~(lr2 > rr[None])).sum()), at_limit=int((acc & (delta == md)).sum()),
                       over_limit=int((el & inside & (lr2 > rr[None]) & (delta > md)).sum()))
    j, k = np.nonzero(acc)
    return dict(j=j, k=k, A=A[j, k], u=u[j, k], w=w[j, k], ls=ls[j, k], lr=lr[j, k], delta=delta[j, k], eligible=elig, d2=d2, v=v, **classes)


def occluded(part, o, d, e1=None, e2=None, nthreads=16):
    """hare_occluded with t_max = 1.0 on the rays (o, d) [m, 3], exclusion words e1, e2 [m] or None."""
    if o.shape[0] == 0:
        return np.zeros(0, bool)
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1))
    kw = {} if e1 is None else dict(excl1=np.ascontiguousarray(e1, np.int32), excl2=np.ascontiguousarray(e2, np.int32))
    ev, _ = part.shoot(rays, nthreads=nthreads, **kw)
    return (ev["hit"] == 1) & (ev["t"] < 1.0)


def diffract(part, pos, power, frame, R, gain, ends, faces, inv_lambda, centers, radii, n_weight, n_bins, bin_len, frac_bits, max_detour, hist,
             det, seen=None, tallies=None, nthreads=16, second_word=True):
    """First-order edge diffraction of the source (pos [3], power [B], frame [3, 3] or None, gain [6, R, R, B] or None with R = 0) over the
    edges (ends [E, 2, 3], faces [E, 2], inv_lambda [B]) at the receivers, standing for n_weight source rays, accumulated into hist
    [K, n_bins, B] or [K, n_bins, B, 4] and det [K, 2] (uint64).  part: the oracle partition that answers the shadow rays.  Returns the
    number of pairs found.  seen (dict, optional) receives pairs()'s dict and blocked [K], and per pair occ_rcv, occ_src, deposited,
    binned.  second_word False restates a build that forgets the second exclusion word (the cases' own check, never the reference)."""
    S = np.asarray(pos, np.float64).reshape(3)
    power = np.asarray(power, np.float64).reshape(-1)
    c = np.asarray(centers, np.float64).reshape(-1, 3)
    rr = np.asarray(radii, np.float64) * np.asarray(radii, np.float64)
    faces = np.asarray(faces, np.int32).reshape(-1, 2)
    lam = np.asarray(inv_lambda, np.float64).reshape(-1)
    B, K = power.shape[0], c.shape[0]
    assert lam.shape[0] == B
    W = np.float64(int(n_weight))
    f = pairs(S, ends, c, radii, max_detour)
    j, k, A, u, w = f["j"], f["k"], f["A"], f["u"], f["w"]
    m = j.size
    blocked = np.zeros(K, bool)
    idx = np.nonzero(f["eligible"])[0]
    blocked[idx] = occluded(part, np.broadcast_to(S, (idx.size, 3)), f["v"][idx], nthreads=nthreads)
    e1, e2 = faces[j, 0], faces[j, 1] if second_word else np.full(m, -1, np.int32)
    occ_r = occluded(part, A, w, e1, e2, nthreads)
    occ_s = occluded(part, A, S[None] - A, e1, e2, nthreads)
    dep = np.nonzero(blocked[k] & ~occ_r & ~occ_s)[0]
    with np.errstate(all="ignore"):
        q = f["ls"][dep] / f["lr"][dep]
        Sx = A[dep] - w[dep] * q[:, None]                                          # S*
        vs = c[k[dep]] - Sx
        d2 = (vs[:, 0] * vs[:, 0] + vs[:, 1] * vs[:, 1]) + vs[:, 2] * vs[:, 2]
        dist = np.sqrt(d2)
        fw = share(rr[k[dep]], d2) * W
        r = 1.0 / (3.0 + 20.0 * ((2.0 * f["delta"][dep])[:, None] * lam[None, :]))    # [m', B]
        xb = dist / np.float64(bin_len)
    g = np.ones((dep.size, B))
    if R and dep.size:
        F, iv, iu, _ = lookup(u[dep], np.eye(3) if frame is None else frame, R)
        g = np.asarray(gain, np.float64).reshape(6, R, R, -1)[F, iv, iu, :]
    binned = (xb >= 0) & (xb < np.float64(n_bins))
    np.add.at(det[:, 0], k[dep][binned], np.uint64(1))
    np.add.at(det[:, 1], k[dep][~binned], np.uint64(1))
    for i in np.nonzero(binned)[0]:
        with np.errstate(all="ignore"):
            val = (((power * g[i]) * r[i]) * fw[i])[:, None]
        vi, di = vs[i], dist[i]

        def arrival():
            return -(vi[0:1] / di), -(vi[1:2] / di), -(vi[2:3] / di)
        ir.deposit(hist, int(k[dep[i]]), np.array([int(np.floor(xb[i]))]), val, frac_bits, arrival, None, tallies)
    if seen is not None:
        deposited, full = np.zeros(m, bool), np.zeros(m, bool)
        deposited[dep] = True
        full[dep] = binned
        seen.update(f, blocked=blocked, occ_rcv=occ_r, occ_src=occ_s, deposited=deposited, binned=full, r=r, dep=dep)
    return m
