"""numpy restatement of diffuse rain in the receive loop (include/hare_hip.h, "receivers", "Diffuse rain"), operation for operation in FP64:
tests/scatter_ref.py's cast-by-cast loop with, in every cast that reflects, each taking-part ray's rain to every receiver -- the shadow
queries run through the oracle partition's shoot (poly_origin1 = Poly_id; occluded = hit && t < 1.0) -- and the receiver step skipped for
the segment behind a diffuse reflection.  The library's results must match it bit for bit."""
import numpy as np

from tests.receiver_ref import quantise, receiver_step
from tests.scatter_ref import choose, normals_of, ray_base, scatter_rays, uniform, weights


def side_normals(d, n):
    """n' = dot3(d, n) > 0 ? -n : n (the side the ray came from)."""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    n = np.asarray(n, np.float64).reshape(-1, 3)
    dn = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    return np.where((dn > 0)[:, None], -n, n)


def rain_step(part, x, nprime, pid, length, Lp, Ea, sg, centers, radii, n_bins, bin_len, frac_bits, hist, det, stats=None, nthreads=16):
    """The rain of m rays that take part: X_Points x [m, 3], side normals n' [m, 3], Poly_id [m], len [m], L' [m], Ea [B, m] and
    sg [B, m] (the sigma rows).  hist [K, n_bins, B] and det [K, 2] are accumulated into.  stats (dict, optional) counts the eligible
    and the occluded queries."""
    centers = np.asarray(centers, np.float64).reshape(-1, 3)
    rr = np.asarray(radii, np.float64) * np.asarray(radii, np.float64)
    with np.errstate(all="ignore"):
        for k in range(centers.shape[0]):
            cx, cy, cz = centers[k]
            vx = cx - x[:, 0]
            vy = cy - x[:, 1]
            vz = cz - x[:, 2]
            d2 = (vx * vx + vy * vy) + vz * vz
            cs = (vx * nprime[:, 0] + vy * nprime[:, 1]) + vz * nprime[:, 2]
            idx = np.nonzero((d2 > rr[k]) & (cs > 0))[0]
            if idx.size == 0:
                continue
            srays = np.stack([x[idx, 0], x[idx, 1], x[idx, 2], vx[idx], vy[idx], vz[idx]], axis=1)
            ev, _ = part.shoot(srays, excl1=np.asarray(pid, np.int32)[idx], nthreads=nthreads)
            occ = (ev["hit"] == 1) & (ev["t"] < 1.0)
            if stats is not None:
                stats["eligible"] = stats.get("eligible", 0) + int(idx.size)
                stats["occluded"] = stats.get("occluded", 0) + int(occ.sum())
            vis = idx[~occ]
            dist = np.sqrt(d2[vis])
            w = (cs[vis] / dist) * (rr[k] / d2[vis])
            xb = (Lp[vis] + dist / length[vis]) / np.float64(bin_len)
            binned = (xb >= 0) & (xb < np.float64(n_bins))
            det[k, 0] += np.uint64(np.count_nonzero(binned))
            det[k, 1] += np.uint64(np.count_nonzero(~binned))
            if binned.any():
                bins = np.floor(xb[binned]).astype(np.int64)
                sel = vis[binned]
                q = quantise((Ea[:, sel] * sg[:, sel]) * w[binned], frac_bits)      # ((Ea * sg) * w) * 2^frac_bits
                for b in range(hist.shape[2]):
                    np.add.at(hist[k, :, b], bins, q[b])


def rain_receive_loop(po, topo, part, rays, bounces, centers, radii, n_bins, bin_len, frac_bits, alpha=None, sigma=None, seed=0,
                      state_in=None, g0=0, rain=True, stats=None, nthreads=16):
    """scatter_ref.scatter_receive_loop with diffuse rain (rain=False: that loop).  Returns (hist [K, n_bins, B], det [K, 2],
    state [1 + B, n], the final rays [n, 6])."""
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    n = rays.shape[0]
    B = 1
    for t in (alpha, sigma):
        if t is not None:
            B = np.asarray(t).shape[1]
    K = np.asarray(centers).reshape(-1, 3).shape[0]
    hist = np.zeros((K, n_bins, B), np.uint64)
    det = np.zeros((K, 2), np.uint64)
    if state_in is None:
        L, E = np.zeros(n), np.ones((B, n))
    else:
        st = np.array(state_in, np.float64).reshape(1 + B, n)
        L, E = st[0].copy(), st[1:].copy()
    normals = normals_of(topo)
    base = ray_base(seed, np.arange(g0, g0 + n, dtype=np.uint64))
    cur = rays.copy()
    e1 = np.full(n, -1, np.int32)
    live = np.ones(n, bool)
    rained = np.zeros(n, bool)              # the segment behind a diffuse reflection: deposited by the rain, not detected
    for c in range(bounces):
        ev = np.zeros(n, po.XEVENT_DTYPE)
        ev["poly_id"] = -1
        if live.any():
            ev_live, _ = part.shoot(cur[live], excl1=e1[live], nthreads=nthreads)
            ev[live] = ev_live
        hit = ev["hit"] == 1
        t_end = np.where(hit, ev["t"], np.inf)
        seen = live & ~rained
        if seen.any():
            receiver_step(cur[seen, :3], cur[seen, 3:], t_end[seen], L[seen], E[:, seen], centers, radii, n_bins, bin_len, frac_bits, hist, det)
        upd = live & hit
        if alpha is not None:
            a = np.asarray(alpha, np.float64)[ev["poly_id"][upd]].T          # [B, m]
            E[:, upd] = E[:, upd] * (1.0 - a)
        L[upd] = L[upd] + ev["t"][upd]
        rained = np.zeros(n, bool)
        if c + 1 < bounces:
            nxt = po.reflect_batch(topo, cur, ev)
            if sigma is not None and upd.any():
                idx = np.nonzero(upd)[0]
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
                        rain_step(part, x, side_normals(d, normals[pid[t]]), pid[t], length, L[ti], E[:, ti], srow[t].T, centers, radii,
                                  n_bins, bin_len, frac_bits, hist, det, stats=stats, nthreads=nthreads)
                    rained[idx[diff]] = True
                E[:, idx] = E[:, idx] * weights(srow, p, diff).T
                di = idx[diff]
                if di.size:
                    nxt[di] = scatter_rays(cur[di], ev[di], normals, base[di], c)
            cur = nxt
        e1 = np.where(upd, ev["poly_id"], -2).astype(np.int32)
        live = upd
    return hist, det, np.concatenate([L[None], E], axis=0), cur
