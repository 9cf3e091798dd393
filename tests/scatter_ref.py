"""numpy restatement of the receive loop's diffuse scattering (include/hare_hip.h, "receivers", "Scattering"): the counter-based RNG, the
diffuse / specular choice, the band weights and the cosine-distributed direction, operation for operation in FP64 (numpy evaluates every
product and sum on its own: no contraction).  tests/receive_ref.py's cast-by-cast loop calls these; the library's results must match it
bit for bit."""
import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)
TRIES = 32


def mix(z):
    """SplitMix64's finaliser on uint64 (arrays or scalars), wrapping mod 2^64."""
    z = np.array(z, dtype=np.uint64, copy=True)
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= M1
        z ^= z >> np.uint64(27)
        z *= M2
        z ^= z >> np.uint64(31)
    return z


def seed_bits(seed):
    """The scene option "scatter_seed" (an int64) read as uint64 bits."""
    return np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)


def ray_base(seed, g):
    """base = mix(mix(S + G) ^ g) for global ray indices g."""
    with np.errstate(over="ignore"):
        s = mix(np.array([seed_bits(seed)], np.uint64) + G)[0]
    return mix(s ^ np.asarray(g, np.uint64))


def uniform(base, c, j):
    """u_j = (double)(mix(base + ((c << 8) | j) * G) >> 11) * 2^-53 for cast c and word j (both may be arrays)."""
    word = (np.asarray(c, np.uint64) << np.uint64(8)) | np.asarray(j, np.uint64)
    with np.errstate(over="ignore"):
        z = mix(np.asarray(base, np.uint64) + word * G)
    return (z >> np.uint64(11)).astype(np.float64) * np.float64(2.0 ** -53)


def choose(sigma_rows, u0):
    """p = (((sigma[0] + sigma[1]) + ...) + sigma[B-1]) / B per row, and diffuse = u0 < p."""
    s = np.asarray(sigma_rows, np.float64)
    p = s[:, 0].copy()
    for b in range(1, s.shape[1]):
        p = p + s[:, b]
    p = p / np.float64(s.shape[1])
    return p, u0 < p


def weights(sigma_rows, p, diffuse):
    """sigma[b] / p for diffuse rays, (1 - sigma[b]) / (1 - p) for the others: [m, B]."""
    s = np.asarray(sigma_rows, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        wd = s / p[:, None]
        ws = (1.0 - s) / (1.0 - p[:, None])
    return np.where(diffuse[:, None], wd, ws)


def disc(base, c):
    """Malley's rejection step: the first (x, y) of u_{1+2t}, u_{2+2t} (t < 32) inside the unit disc; (0, 0, 0) when none is."""
    m = np.asarray(base).shape[0]
    x, y, r2 = np.zeros(m), np.zeros(m), np.zeros(m)
    todo = np.ones(m, bool)
    for t in range(TRIES):
        if not todo.any():
            break
        idx = np.nonzero(todo)[0]
        xt = 2.0 * uniform(base[idx], c if np.ndim(c) == 0 else np.asarray(c)[idx], 1 + 2 * t) - 1.0
        yt = 2.0 * uniform(base[idx], c if np.ndim(c) == 0 else np.asarray(c)[idx], 2 + 2 * t) - 1.0
        rt = xt * xt + yt * yt
        ok = rt < 1.0
        x[idx[ok]], y[idx[ok]], r2[idx[ok]] = xt[ok], yt[ok], rt[ok]
        todo[idx[ok]] = False
    return x, y, r2


def direction(d, n, x, y, r2):
    """The diffuse direction of rays d [m, 3] off polygons of normal n [m, 3] from the disc point (x, y, r2): w * |d|."""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    n = np.asarray(n, np.float64).reshape(-1, 3)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    dn = (dx * n[:, 0] + dy * n[:, 1]) + dz * n[:, 2]                       # hare_math.h dot3
    flip = dn > 0
    nx = np.where(flip, -n[:, 0], n[:, 0])
    ny = np.where(flip, -n[:, 1], n[:, 1])
    nz = np.where(flip, -n[:, 2], n[:, 2])
    z = np.sqrt(1.0 - r2)
    sg = np.copysign(1.0, nz)
    a = -1.0 / (sg + nz)
    b = (nx * ny) * a
    t1 = (1.0 + ((sg * nx) * nx) * a, sg * b, -(sg * nx))
    t2 = (b, sg + (ny * ny) * a, -ny)
    nn = (nx, ny, nz)
    w = [(x * t1[i] + y * t2[i]) + z * nn[i] for i in range(3)]
    ln = np.sqrt((dx * dx + dy * dy) + dz * dz)
    return np.stack([w[0] * ln, w[1] * ln, w[2] * ln], axis=1), np.stack(nn, axis=1)


def scatter_rays(rays, ev, normals, base, c):
    """Diffuse rays: origin the X_Point, direction from direction().  rays [m, 6], ev [m] events, normals [P, 3]."""
    x, y, r2 = disc(base, c)
    d, _ = direction(rays[:, 3:], normals[ev["poly_id"]], x, y, r2)
    out = np.empty_like(rays)
    out[:, 0], out[:, 1], out[:, 2] = ev["x"], ev["y"], ev["z"]
    out[:, 3:] = d
    return out


def normals_of(topo):
    """PolyRec::n of every polygon: the normals the oracle's reflection uses (Topology.Normal)."""
    return np.asarray(topo.normals, np.float64).reshape(-1, 3)
