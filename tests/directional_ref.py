"""numpy restatement of the directional receivers (include/hare_hip.h, "receivers", "Directional"), operation for operation in FP64:
the receiver step and the rain deposit with four channels per histogram word -- W, the omni word of tests/receiver_ref.py and
tests/rain_ref.py, and X, Y, Z, the add weighted by the unit vector towards where the sound came from, as int64 in two's complement --
inside one cast-by-cast loop that serves the three receive loops: specular (no table), scattering (tests/scatter_ref.py's choice, weights
and directions, called unchanged) and diffuse rain (tests/rain_ref.py's eligibility, shadow queries and suppression, restated here
because the deposit sits inside its step).  numpy evaluates every product, quotient and sum on its own (no contraction) and its sqrt and
division are correctly rounded, so the library's results must match it bit for bit."""
import numpy as np

from tests.rain_ref import side_normals
from tests.receiver_ref import TWO63
from tests.scatter_ref import choose, normals_of, ray_base, scatter_rays, uniform, weights

TWO62 = 4611686018427387904.0


def magnitude(v, frac_bits):
    """m_b: v * 2^frac_bits; 0 unless > 0; min(., 2^63) -- the double that q_b is the rint of."""
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.asarray(v, np.float64) * np.float64(2.0 ** int(frac_bits))
        m = np.where(m > 0, m, 0.0)
        return np.minimum(m, TWO63)


def signed_words(m, a):
    """s_i = (int64) rint(min(max(m * a_i, -2^62), 2^62)), 0 for NaN, as the uint64 word that is added."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = m * a
        v = np.where(v == v, v, 0.0)
        v = np.minimum(np.maximum(v, -TWO62), TWO62)
    return np.rint(v).astype(np.int64).view(np.uint64)


def add_words(hist, k, bins, m, a, counts=None):
    """hist[k, bin, b, :] += (rint(m_b), s_0, s_1, s_2) for every add: m [B, m'], a three arrays [m'] (the arrival vector).
    counts [K, n_bins] (optional) collects the number of adds into each (receiver, bin): the same for every band and channel."""
    if counts is not None:
        np.add.at(counts[k], bins, 1)
    with np.errstate(over="ignore"):
        for b in range(hist.shape[2]):
            np.add.at(hist[k, :, b, 0], bins, np.rint(m[b]).astype(np.uint64))
            for i in range(3):
                np.add.at(hist[k, :, b, 1 + i], bins, signed_words(m[b], a[i]))


def receiver_step_dir(o, d, t_end, L, E, centers, radii, n_bins, bin_len, frac_bits, hist, det, counts=None):
    """tests/receiver_ref.py's receiver_step with the four channels: hist [K, n_bins, B, 4].  a is one vector per ray, the same for
    every receiver: len = sqrt((dx*dx + dy*dy) + dz*dz), a = (-(dx / len), -(dy / len), -(dz / len))."""
    o = np.asarray(o, np.float64).reshape(-1, 3)
    d = np.asarray(d, np.float64).reshape(-1, 3)
    E = np.asarray(E, np.float64).reshape(hist.shape[2], -1)
    centers = np.asarray(centers, np.float64).reshape(-1, 3)
    r2 = np.asarray(radii, np.float64) * np.asarray(radii, np.float64)
    ox, oy, oz = o[:, 0], o[:, 1], o[:, 2]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        dd = (dx * dx + dy * dy) + dz * dz
        ln = np.sqrt(dd)
        a = (-(dx / ln), -(dy / ln), -(dz / ln))
        for k in range(centers.shape[0]):
            cx, cy, cz = centers[k]
            wx = cx - ox
            wy = cy - oy
            wz = cz - oz
            s = ((wx * dx + wy * dy) + wz * dz) / dd
            qx = (ox + dx * s) - cx
            qy = (oy + dy * s) - cy
            qz = (oz + dz * s) - cz
            detected = (s >= 0) & (s < t_end) & (((qx * qx + qy * qy) + qz * qz) < r2[k])
            x = (L + s) / np.float64(bin_len)
            binned = detected & (x >= 0) & (x < np.float64(n_bins))
            det[k, 0] += np.uint64(np.count_nonzero(binned))
            det[k, 1] += np.uint64(np.count_nonzero(detected & ~binned))
            if binned.any():
                bins = np.floor(x[binned]).astype(np.int64)
                add_words(hist, k, bins, magnitude(E[:, binned], frac_bits), [c[binned] for c in a], counts)


def rain_step_dir(part, x, nprime, pid, length, Lp, Ea, sg, centers, radii, n_bins, bin_len, frac_bits, hist, det, stats=None, nthreads=16,
                  counts=None):
    """tests/rain_ref.py's rain_step with the four channels: a = (-(vx / dist), -(vy / dist), -(vz / dist)) per deposit."""
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
                m = magnitude((Ea[:, sel] * sg[:, sel]) * w[binned], frac_bits)      # ((Ea * sg) * w) * 2^frac_bits
                db = dist[binned]
                add_words(hist, k, bins, m, (-(vx[sel] / db), -(vy[sel] / db), -(vz[sel] / db)), counts)


def directional_receive_loop(po, topo, part, rays, bounces, centers, radii, n_bins, bin_len, frac_bits, alpha=None, sigma=None, seed=0,
                             state_in=None, g0=0, rain=False, stats=None, nthreads=16, counts=None):
    """The receive loop with HARE_RECEIVE_DIRECTIONAL, cast by cast with part.shoot (an oracle partition): specular without a table,
    scattering with one, diffuse rain with rain=True (which, as in the library, changes nothing without a table).
    counts: an int64 array [K, n_bins] that collects the adds per (receiver, bin), or None.
    Returns (hist [K, n_bins, B, 4] uint64, det [K, 2], state [1 + B, n], the final rays [n, 6])."""
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    n = rays.shape[0]
    B = 1
    for t in (alpha, sigma):
        if t is not None:
            B = np.asarray(t).shape[1]
    K = np.asarray(centers).reshape(-1, 3).shape[0]
    hist = np.zeros((K, n_bins, B, 4), np.uint64)
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
            receiver_step_dir(cur[seen, :3], cur[seen, 3:], t_end[seen], L[seen], E[:, seen], centers, radii, n_bins, bin_len, frac_bits,
                              hist, det, counts)
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
                        rain_step_dir(part, x, side_normals(d, normals[pid[t]]), pid[t], length, L[ti], E[:, ti], srow[t].T, centers, radii,
                                      n_bins, bin_len, frac_bits, hist, det, stats=stats, nthreads=nthreads, counts=counts)
                    rained[idx[diff]] = True
                E[:, idx] = E[:, idx] * weights(srow, p, diff).T
                di = idx[diff]
                if di.size:
                    nxt[di] = scatter_rays(cur[di], ev[di], normals, base[di], c)
            cur = nxt
        e1 = np.where(upd, ev["poly_id"], -2).astype(np.int32)
        live = upd
    return hist, det, np.concatenate([L[None], E], axis=0), cur

