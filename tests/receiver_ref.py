"""numpy restatement of the receiver step and the receive loop (include/hare_hip.h, "receivers"), operation for operation in FP64:
numpy evaluates every product and sum on its own (no contraction), in the order written here, so the library's results must match it bit
for bit."""
import numpy as np

TWO63 = 9223372036854775808.0


def quantise(E, frac_bits):
    """q_b = E[b] * 2^frac_bits; 0 unless q_b > 0; min(q_b, 2^63); rint -> uint64."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.asarray(E, np.float64) * np.float64(2.0 ** int(frac_bits))
        q = np.where(q > 0, q, 0.0)
        q = np.minimum(q, TWO63)
    return np.rint(q).astype(np.uint64)


def receiver_step(o, d, t_end, L, E, centers, radii, n_bins, bin_len, frac_bits, hist, det):
    """One cast's receiver step for the live rays given: o, d [m, 3]; t_end [m] (+inf for a miss); L [m]; E [B, m].
    hist [K, n_bins, B] and det [K, 2] (uint64) are accumulated into (wrapping mod 2^64)."""
    o = np.asarray(o, np.float64).reshape(-1, 3)
    d = np.asarray(d, np.float64).reshape(-1, 3)
    E = np.asarray(E, np.float64).reshape(hist.shape[2], -1)
    centers = np.asarray(centers, np.float64).reshape(-1, 3)
    r2 = np.asarray(radii, np.float64) * np.asarray(radii, np.float64)
    ox, oy, oz = o[:, 0], o[:, 1], o[:, 2]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        dd = (dx * dx + dy * dy) + dz * dz
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
                q = quantise(E[:, binned], frac_bits)              # [B, m']
                for b in range(hist.shape[2]):
                    np.add.at(hist[k, :, b], bins, q[b])


def receive_loop(po, topo, rays, events, centers, radii, n_bins, bin_len, frac_bits, alpha=None, state_in=None):
    """The receive loop from the bounce loop's events of every cast (events [bounces, n], e.g. tests.helpers.oracle_bounce_loop):
    the rays of each cast are rebuilt with the oracle's reflection.  Returns (hist [K, n_bins, B], det [K, 2], state [1 + B, n])."""
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    n = rays.shape[0]
    B = 1 if alpha is None else np.asarray(alpha).shape[1]
    K = np.asarray(centers).reshape(-1, 3).shape[0]
    hist = np.zeros((K, n_bins, B), np.uint64)
    det = np.zeros((K, 2), np.uint64)
    if state_in is None:
        L = np.zeros(n)
        E = np.ones((B, n))
    else:
        st = np.array(state_in, np.float64).reshape(1 + B, n)
        L, E = st[0].copy(), st[1:].copy()
    cur = rays.copy()
    live = np.ones(n, bool)
    for c in range(events.shape[0]):
        ev = events[c]
        hit = ev["hit"] == 1
        t_end = np.where(hit, ev["t"], np.inf)
        if live.any():
            receiver_step(cur[live, :3], cur[live, 3:], t_end[live], L[live], E[:, live], centers, radii, n_bins, bin_len, frac_bits, hist, det)
        upd = live & hit
        if alpha is not None:
            a = np.asarray(alpha, np.float64)[ev["poly_id"][upd]].T          # [B, m]
            E[:, upd] = E[:, upd] * (1.0 - a)
        L[upd] = L[upd] + ev["t"][upd]
        if c + 1 < events.shape[0]:
            cur = po.reflect_batch(topo, cur, ev)
        live = upd
    return hist, det, np.concatenate([L[None], E], axis=0)
