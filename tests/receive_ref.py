"""numpy restatement of the receive loop (include/hare_hip.h, "receivers"), operation for operation in FP64: the receiver step, the rain
step ("Diffuse rain"), the deposit in its omni and its directional ("Directional") form, the termination rules ("Termination"), and the
ONE cast-by-cast loop that serves every mode -- specular (no table), scattering (tests/scatter_ref.py's RNG, choice, weights and
directions) and diffuse rain, each with one word or four channels per band, with or without the rules, over the linear receiver loop or
the candidates of a receiver map ("Receiver maps": the grid and the visit rule are tests/receive_map_ref.py's).  A feature of the loop
is added here, once; tests/golden/receive_reference_digests.json pins what the loop returns (tests/test_receive_reference_pinned.py).
numpy evaluates every product, quotient and sum on its own (no contraction), in the order written here, and
its sqrt and division are correctly rounded, so the library's results must match it bit for bit."""
import numpy as np

from tests.scatter_ref import choose, normals_of, ray_base, scatter_rays, uniform, weights

TWO63 = 9223372036854775808.0
TWO62 = 4611686018427387904.0


def magnitude(v, frac_bits):
    """m_b: v * 2^frac_bits; 0 unless > 0; min(., 2^63) -- the double that q_b is the rint of."""
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.asarray(v, np.float64) * np.float64(2.0 ** int(frac_bits))
        m = np.where(m > 0, m, 0.0)
        return np.minimum(m, TWO63)


def quantise(E, frac_bits):
    """q_b = rint(m_b) -> uint64."""
    return np.rint(magnitude(E, frac_bits)).astype(np.uint64)


def signed_words(m, a):
    """s_i = (int64) rint(min(max(m * a_i, -2^62), 2^62)), 0 for NaN, as the uint64 word that is added."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = m * a
        v = np.where(v == v, v, 0.0)
        v = np.minimum(np.maximum(v, -TWO62), TWO62)
    return np.rint(v).astype(np.int64).view(np.uint64)


TALLIES = ("saturated", "zeroed", "zeroed_nan", "zeroed_negative", "zeroed_zero", "zeroed_negative_zero", "ties", "round_to_zero",
           "dir_clamped", "dir_nan", "wrapped")


def tally(tallies, hist, k, bins, v, m, a, frac_bits):
    """The classes of the definition's edge cases that one deposit call went through, added to the dict `tallies` (TALLIES): adds with
    m == 2^63 (saturated); adds whose product v * 2^frac_bits was NaN, < 0, +0.0 or -0.0 and became 0 (zeroed, and each on its own);
    ties (m - floor(m) == 0.5); products > 0 that round to 0; directional words clamped at +-2^62 and zeroed for NaN; and, counted
    before the adds are made, the omni words whose sum with this call's adds passes 2^64 (wrapped)."""
    with np.errstate(invalid="ignore", over="ignore"):
        raw = np.asarray(v, np.float64) * np.float64(2.0 ** int(frac_bits))
        new = {"saturated": m == TWO63, "zeroed": ~(raw > 0), "zeroed_nan": raw != raw, "zeroed_negative": raw < 0,
               "zeroed_zero": (raw == 0) & ~np.signbit(raw), "zeroed_negative_zero": (raw == 0) & np.signbit(raw),
               "ties": m - np.floor(m) == 0.5, "round_to_zero": (raw > 0) & (np.rint(m) == 0)}
        if a is not None:
            w = np.stack([m * a[i] for i in range(3)])
            new["dir_clamped"] = np.abs(w) > TWO62
            new["dir_nan"] = w != w
    for name in TALLIES:
        tallies[name] = tallies.get(name, 0) + int(np.count_nonzero(new.get(name, False)))
    # exact sums in two 32-bit halves (fewer than 2^31 adds per call): does old + adds reach 2^64?
    ub, inv = np.unique(bins, return_inverse=True)
    lo32 = np.uint64(0xFFFFFFFF)
    for b in range(hist.shape[2]):
        q = np.rint(m[b]).astype(np.uint64)
        hi, lo = np.zeros(ub.size, np.uint64), np.zeros(ub.size, np.uint64)
        np.add.at(hi, inv, q >> np.uint64(32))
        np.add.at(lo, inv, q & lo32)
        old = hist[k, ub, b, 0] if hist.ndim == 4 else hist[k, ub, b]
        top = (old >> np.uint64(32)) + hi + (((old & lo32) + lo) >> np.uint64(32))
        tallies["wrapped"] += int(np.count_nonzero(top >> np.uint64(32)))


def deposit(hist, k, bins, v, frac_bits, arrival, counts=None, tallies=None):
    """The one thing the omni and the directional form differ in.  v [B, m'] is the energy of every add.
    hist [K, n_bins, B]: hist[k, bin, b] += q_b.  hist [K, n_bins, B, 4]: hist[k, bin, b, :] += (q_b, s_0, s_1, s_2) with
    arrival() -> three arrays [m'], the unit vector towards where the sound came from (not evaluated for the omni form).
    counts [K, n_bins] (optional) collects the number of adds into each (receiver, bin): the same for every band and channel.
    tallies (dict, optional) collects how many adds went through each edge case of the definition (tally, above)."""
    if counts is not None:
        np.add.at(counts[k], bins, 1)
    m = magnitude(v, frac_bits)
    a = arrival() if hist.ndim == 4 else None
    if tallies is not None:
        tally(tallies, hist, k, bins, v, m, a, frac_bits)
    with np.errstate(over="ignore"):
        for b in range(hist.shape[2]):
            if a is None:
                np.add.at(hist[k, :, b], bins, np.rint(m[b]).astype(np.uint64))
                continue
            np.add.at(hist[k, :, b, 0], bins, np.rint(m[b]).astype(np.uint64))
            for i in range(3):
                np.add.at(hist[k, :, b, 1 + i], bins, signed_words(m[b], a[i]))


def receiver_step(o, d, t_end, L, E, centers, radii, n_bins, bin_len, frac_bits, hist, det, counts=None, tallies=None, cand=None):
    """One cast's receiver step for the live rays given: o, d [m, 3]; t_end [m] (+inf for a miss); L [m]; E [B, m].
    hist [K, n_bins, B] or [K, n_bins, B, 4] and det [K, 2] (uint64) are accumulated into (wrapping mod 2^64).  The arrival vector of
    the directional form is one per ray, the same for every receiver: len = sqrt((dx*dx + dy*dy) + dz*dz),
    a = (-(dx / len), -(dy / len), -(dz / len)).  cand (bool [m, K], optional): the candidate mask of a receiver map -- for receiver k
    only the rays with cand[:, k] take part, the others are out before anything is counted (detection is per ray and receiver, and the
    adds are integer sums mod 2^64: the result is that of the step run per receiver on its candidates alone)."""
    o = np.asarray(o, np.float64).reshape(-1, 3)
    d = np.asarray(d, np.float64).reshape(-1, 3)
    E = np.asarray(E, np.float64).reshape(hist.shape[2], -1)
    centers = np.asarray(centers, np.float64).reshape(-1, 3)
    r2 = np.asarray(radii, np.float64) * np.asarray(radii, np.float64)
    ox, oy, oz = o[:, 0], o[:, 1], o[:, 2]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        dd = (dx * dx + dy * dy) + dz * dz
        for k in range(centers.shape[0]) if cand is None else np.nonzero(cand.any(axis=0))[0]:
            cx, cy, cz = centers[k]
            wx = cx - ox
            wy = cy - oy
            wz = cz - oz
            s = ((wx * dx + wy * dy) + wz * dz) / dd
            qx = (ox + dx * s) - cx
            qy = (oy + dy * s) - cy
            qz = (oz + dz * s) - cz
            detected = (s >= 0) & (s < t_end) & (((qx * qx + qy * qy) + qz * qz) < r2[k])
            if cand is not None:
                detected &= cand[:, k]
            x = (L + s) / np.float64(bin_len)
            binned = detected & (x >= 0) & (x < np.float64(n_bins))
            det[k, 0] += np.uint64(np.count_nonzero(binned))
            det[k, 1] += np.uint64(np.count_nonzero(detected & ~binned))
            if binned.any():
                bins = np.floor(x[binned]).astype(np.int64)

                def arrival():
                    ln = np.sqrt(dd[binned])
                    return -(dx[binned] / ln), -(dy[binned] / ln), -(dz[binned] / ln)
                deposit(hist, k, bins, E[:, binned], frac_bits, arrival, counts, tallies)


receiver_step_dir = receiver_step           # the directional form is chosen by hist's shape


def side_normals(d, n):
    """n' = dot3(d, n) > 0 ? -n : n (the side the ray came from)."""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    n = np.asarray(n, np.float64).reshape(-1, 3)
    dn = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    return np.where((dn > 0)[:, None], -n, n)


def rain_step(part, x, nprime, pid, length, Lp, Ea, sg, centers, radii, n_bins, bin_len, frac_bits, hist, det, stats=None, nthreads=16,
              counts=None, tallies=None):
    """The rain of m rays that take part: X_Points x [m, 3], side normals n' [m, 3], Poly_id [m], len [m], L' [m], Ea [B, m] and
    sg [B, m] (the sigma rows).  The shadow queries run through the oracle partition's shoot (poly_origin1 = Poly_id; occluded =
    hit && t < 1.0).  hist and det are accumulated into as in receiver_step; the arrival vector of the directional form is
    a = (-(vx / dist), -(vy / dist), -(vz / dist)) per deposit.  stats (dict, optional) counts the eligible and the occluded queries."""
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

                def arrival():
                    db = dist[binned]
                    return -(vx[sel] / db), -(vy[sel] / db), -(vz[sel] / db)
                deposit(hist, k, bins, (Ea[:, sel] * sg[:, sel]) * w[binned], frac_bits, arrival, counts,
                        tallies)                                        # ((Ea * sg) * w) * 2^frac_bits


ROULETTE_WORD = 65                       # u_65: scattering draws j = 0 .. 64


def decide(L, E, base, c, n_bins, bin_len, time_limit, floor_bits, roulette):
    """The termination rules ("Termination": the time limit HARE_RECEIVE_TIME_LIMIT, the energy floor "receive_floor_bits" and its Russian
    roulette "receive_roulette") for m rays that hit in cast c and would be reflected: L [m] and E [B, m] AFTER the cast's state update,
    base [m] the RNG's per-ray base.  Returns (cut_time [m] bool, cut_floor [m] bool, boosted [m] bool, E' [B, m]): E' is E but for the
    roulette's survivors, whose bands are divided by ps."""
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


def receive_loop(po, topo, part, rays, bounces, centers, radii, n_bins, bin_len, frac_bits, alpha=None, sigma=None, seed=0, state_in=None,
                 g0=0, rain=False, directional=False, keep_rays_after=None, stats=None, counts=None, nthreads=16, events=None,
                 tallies=None, excl1=None, excl2=None, last_events=None, time_limit=False, floor_bits=0, roulette=False, visit=None,
                 per_cast=None, share=None):
    """The receive loop, cast by cast: part.shoot (an oracle partition) on the live rays, the receiver step, the state update, then (but
    behind the last cast) the choice, the rain, the weights, the reflection -- specular rays with the oracle's reflection, diffuse
    ones with tests/scatter_ref.py's -- and the termination rules.  sigma: the scattering table (None: specular).  rain: diffuse rain,
    with the receiver step skipped for the segment behind a diffuse reflection (as in the library, it changes nothing without a table).
    directional: four channels per band.  g0: the global index of ray 0.  counts: an int64 array [K, n_bins] that collects the adds per
    (receiver, bin), or None.  events [bounces, n] (e.g. tests.helpers.oracle_bounce_loop): replay these recorded events of every cast
    instead of shooting.  tallies: deposit's dict of edge-case classes, or None.  excl1, excl2 [n]: poly_origin1 / poly_origin2 of the
    first cast (default: none).  last_events: a list that receives the last cast's events [n] (a miss record for a retired ray), or None.
    time_limit, floor_bits, roulette: the rules of decide(), above (default: none).  visit: a callable (o, d, t_end) -> bool [m, K], the
    candidate mask of a receiver map (tests.receive_map_ref.candidates on a grid), or None for the linear loop; with rain and a table it
    is refused, as by the library.  per_cast: a dict that receives four int64 arrays [bounces] -- "live" (rays that took part in the
    cast), "time" and "floor" (rays the rule retired in it), "boosted" (roulette survivors) -- or None.  share: a list that receives
    (candidate pairs, rays x receivers) of every receiver step under `visit`, or None.
    Returns (hist [K, n_bins, B] or [K, n_bins, B, 4] uint64, det [K, 2], state [1 + B, n], the rays [n, 6] behind cast
    `keep_rays_after`, or the final ones)."""
    if visit is not None and rain and sigma is not None:
        raise ValueError("diffuse rain with a receiver map and a scattering table")
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
    rained = np.zeros(n, bool)              # the segment behind a diffuse reflection: deposited by the rain, not detected
    kept = None
    if per_cast is not None:
        per_cast.update({k: np.zeros(bounces, np.int64) for k in ("live", "time", "floor", "boosted")})
    for c in range(bounces):
        if per_cast is not None:
            per_cast["live"][c] = int(live.sum())
        ev = np.zeros(n, po.XEVENT_DTYPE)
        ev["poly_id"] = -1
        if live.any():
            ev[live] = events[c][live] if events is not None else part.shoot(cur[live], excl1=e1[live], excl2=None if e2 is None else e2[live],
                                                                             nthreads=nthreads)[0]
        hit = ev["hit"] == 1
        t_end = np.where(hit, ev["t"], np.inf)
        seen = live & ~rained
        if seen.any():
            cand = None
            if visit is not None:
                cand = visit(cur[seen, :3], cur[seen, 3:], t_end[seen])
                if share is not None:
                    share.append((int(cand.sum()), cand.size))
            receiver_step(cur[seen, :3], cur[seen, 3:], t_end[seen], L[seen], E[:, seen], centers, radii, n_bins, bin_len, frac_bits,
                          hist, det, counts, tallies, cand)
        upd = live & hit
        if alpha is not None:
            a = np.asarray(alpha, np.float64)[ev["poly_id"][upd]].T          # [B, m]
            with np.errstate(invalid="ignore"):                              # inf * 0
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
                        rain_step(part, x, side_normals(d, normals[pid[t]]), pid[t], length, L[ti], E[:, ti], srow[t].T, centers, radii,
                                  n_bins, bin_len, frac_bits, hist, det, stats=stats, nthreads=nthreads, counts=counts, tallies=tallies)
                    rained[idx[diff]] = True
                with np.errstate(invalid="ignore", over="ignore"):
                    E[:, idx] = E[:, idx] * weights(srow, p, diff).T
                di = idx[diff]
                if di.size:
                    nxt[di] = scatter_rays(cur[di], ev[di], normals, base[di], c)
            # termination: behind the state update; a retired ray keeps the ray the cast received and is treated as a miss from here
            if (time_limit or floor_bits) and idx.size:
                ct, cf, boosted, E[:, idx] = decide(L[idx], E[:, idx], base[idx], c, n_bins, bin_len, time_limit, floor_bits, roulette)
                gone = idx[ct | cf]
                nxt[gone] = cur[gone]
                goes_on = upd.copy()
                goes_on[gone] = False
                rained[gone] = False
                if per_cast is not None:
                    for name, v in (("time", ct), ("floor", cf), ("boosted", boosted)):
                        per_cast[name][c] = int(v.sum())
            cur = nxt
            if keep_rays_after == c:
                kept = cur.copy()
        e1 = np.where(goes_on, ev["poly_id"], -2).astype(np.int32)
        e2 = None
        live = goes_on
        if last_events is not None and c + 1 == bounces:
            last_events.append(ev)
    return hist, det, np.concatenate([L[None], E], axis=0), cur if keep_rays_after is None else kept


def replay_loop(po, topo, rays, events, centers, radii, n_bins, bin_len, frac_bits, alpha=None, state_in=None):
    """The specular receive loop from the bounce loop's recorded events of every cast (events [bounces, n]): receive_loop with nothing
    shot.  Returns (hist [K, n_bins, B], det [K, 2], state [1 + B, n])."""
    return receive_loop(po, topo, None, rays, events.shape[0], centers, radii, n_bins, bin_len, frac_bits, alpha=alpha, state_in=state_in,
                        events=events)[:3]
