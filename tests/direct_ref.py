"""numpy restatement of the direct sound (include/hare_hip.h, "receivers", "Direct sound"): one visibility query and one deposit per
receiver, from the scene's source, operation for operation in FP64.  Written on what exists: tests/source_ref.py's cube-map lookup for
the gains, tests/receive_ref.py's deposit for the quantising and the channels, and the oracle partition's shoot for the occlusion, as
receive_ref.rain_step does it.  hare_direct_device's histogram and detections must match direct() byte for byte.  cases() are the device
cases of tests/test_gpu_direct.py; tests/test_direct_ref.py asserts on the CPU that they hold what they claim to hold."""
import dataclasses

import numpy as np

from tests.receive_cases import mesh_of
from tests.receive_ref import deposit
from tests.source_ref import lookup, powers, rotation, table


def share(rr, d2):
    """f = (0.5 * x) / (1.0 + sqrt(1.0 - x)) with x = rr / d2: the share of the directions that pass through the sphere,
    (1 - cos theta) / 2 with sin^2 theta = x, without cancellation."""
    x = rr / d2
    return (0.5 * x) / (1.0 + np.sqrt(1.0 - x))


def direct(part, pos, power, frame, R, gain, centers, radii, n_weight, n_bins, bin_len, frac_bits, hist, det, seen=None, tallies=None,
           nthreads=16):
    """The direct sound of the source (pos [3], power [B], frame [3, 3] or None, gain [6, R, R, B] or None with R = 0) at the receivers,
    standing for n_weight source rays, accumulated into hist [K, n_bins, B] or [K, n_bins, B, 4] and det [K, 2] (uint64).  part: the
    oracle partition that answers the shadow rays (occluded = hit && t < 1.0, nothing excluded).  seen (dict, optional) receives bool
    arrays [K] -- eligible, occluded, binned, edge (dist / bin_len a whole number) -- and `faces`, the set of cube faces read.
    tallies: receive_ref.deposit's dict of edge-case classes."""
    pos = np.asarray(pos, np.float64).reshape(3)
    power = np.asarray(power, np.float64).reshape(-1)
    centers = np.asarray(centers, np.float64).reshape(-1, 3)
    rr = np.asarray(radii, np.float64) * np.asarray(radii, np.float64)
    K = centers.shape[0]
    W = np.float64(int(n_weight))
    vx = centers[:, 0] - pos[0]
    vy = centers[:, 1] - pos[1]
    vz = centers[:, 2] - pos[2]
    d2 = (vx * vx + vy * vy) + vz * vz
    elig = d2 > rr
    idx = np.nonzero(elig)[0]
    occ = np.zeros(K, bool)
    if idx.size:
        srays = np.stack([np.full(idx.size, pos[0]), np.full(idx.size, pos[1]), np.full(idx.size, pos[2]), vx[idx], vy[idx], vz[idx]], axis=1)
        ev, _ = part.shoot(np.ascontiguousarray(srays), nthreads=nthreads)
        occ[idx] = (ev["hit"] == 1) & (ev["t"] < 1.0)
    vis = np.nonzero(elig & ~occ)[0]
    dist = np.sqrt(d2[vis])
    fw = share(rr[vis], d2[vis]) * W
    g = np.ones((vis.size, power.shape[0]))
    faces = set()
    if R:
        F, iv, iu, paths = lookup(np.stack([vx[vis], vy[vis], vz[vis]], axis=1), np.eye(3) if frame is None else frame, R)
        g = np.asarray(gain, np.float64).reshape(6, R, R, -1)[F, iv, iu, :]
        faces = paths["faces"] if vis.size else set()
    xb = dist / np.float64(bin_len)
    binned = (xb >= 0) & (xb < np.float64(n_bins))
    np.add.at(det[:, 0], vis[binned], np.uint64(1))
    np.add.at(det[:, 1], vis[~binned], np.uint64(1))
    for j in np.nonzero(binned)[0]:
        k = int(vis[j])
        v = ((power * g[j]) * fw[j])[:, None]                                    # ((power[b] * g_b) * (f * W)), then * 2^frac_bits

        def arrival():
            return -(vx[k:k + 1] / dist[j]), -(vy[k:k + 1] / dist[j]), -(vz[k:k + 1] / dist[j])
        deposit(hist, k, np.array([int(np.floor(xb[j]))]), v, frac_bits, arrival, None, tallies)
    if seen is not None:
        full = np.zeros(K, bool)
        full[vis] = binned
        edge = np.zeros(K, bool)
        edge[vis] = xb == np.floor(xb)
        seen.update(eligible=elig, occluded=occ, binned=full, edge=edge, faces=faces)


# ---- the device cases (tests/test_gpu_direct.py), shared with the CPU check that they are not vacuous (tests/test_direct_ref.py)
POS = (3.0, 2.0, 1.5)                   # in the partition room (tests.receive_cases.partition_room): its wall x = 5, y = 0 .. 4.2 hides the far side
PARTITIONS = (("voxel", 8), ("octree", 4, 8), ("kdtree", 8, 6))


@dataclasses.dataclass
class DirectCase:
    name: str
    partition: tuple
    K: int
    map: bool                            # the receivers as a receiver map (set_receiver_map)
    B: int
    R: int                               # the table's resolution (0: none); read in source_ref.rotation()
    frac_bits: int
    n_bins: int
    bin_len: float
    directional: bool
    n_weight: int
    scene: tuple = ("room",)

    @property
    def shape(self):
        return (self.K, self.n_bins, self.B, 4) if self.directional else (self.K, self.n_bins, self.B)

    def receivers(self):
        """centers [K, 3], radii [K].  The first five are placed: 0 straight above the source at a distance of exactly 1 (dist / bin_len a
        whole number for every bin_len 2^-j), 1 around the source (not eligible), 2 behind the wall (occluded), 3 in the far corner of
        the source's side (unbinned in a short histogram), 4 small and far (a product that rounds to 0 at frac_bits 0).  The others lie
        about the room, on both sides of the wall."""
        rng = np.random.default_rng(77 + self.K)
        _, _, size = mesh_of(self.scene)
        c = rng.uniform(0.05, 0.95, (self.K, 3)) * np.asarray(size)
        r = rng.uniform(0.1, 0.4, self.K)
        placed = [((POS[0], POS[1], POS[2] + 1.0), 0.25), ((POS[0] + 0.125, POS[1], POS[2]), 0.5), ((7.0, 2.0, 1.5), 0.3),
                  ((0.5, 6.5, 3.5), 0.3), ((1.0, 6.0, 0.5), 0.0625)]
        for k, (ck, rk) in enumerate(placed[:self.K]):
            c[k], r[k] = ck, rk
        return np.ascontiguousarray(c), r

    def source(self):
        """(pos, power [B], frame or None, R, gain or None)."""
        return (np.array(POS), powers(self.B), rotation() if self.R else None, self.R, table(self.R, self.B) if self.R else None)


def cases():
    """Every partition; K = 1, 3, 64, 255, 256 linear, 257 and 4 096 as a map; B = 1, 3, 8; R = 0, 1, 4 in a rotated frame; frac_bits 0, 40,
    62; one bin and 4 096 bins; one and four channels; n_weight 1, 4 097, 2^40."""
    C = DirectCase
    out = [C("K1", PARTITIONS[0], 1, False, 1, 0, 40, 64, 0.125, False, 4097),
           C("K3-dir", PARTITIONS[1], 3, False, 3, 1, 0, 8, 0.5, True, 1),
           C("K64", PARTITIONS[2], 64, False, 8, 4, 62, 64, 0.125, False, 2 ** 40),
           C("K255-dir", PARTITIONS[0], 255, False, 3, 4, 40, 4096, 2.0 ** -8, True, 4097),
           C("K256", PARTITIONS[1], 256, False, 8, 0, 0, 1, 4.0, False, 1),
           C("K256-dir-sat", PARTITIONS[2], 256, False, 1, 1, 62, 1, 4.0, True, 2 ** 40),
           C("map257", PARTITIONS[0], 257, True, 3, 4, 0, 8, 0.5, False, 4097),
           C("map257-dir", PARTITIONS[2], 257, True, 8, 0, 40, 64, 0.125, True, 1),
           C("map4096", PARTITIONS[1], 4096, True, 1, 4, 40, 64, 0.125, False, 2 ** 40),
           C("map4096-dir", PARTITIONS[0], 4096, True, 3, 1, 62, 16, 0.5, True, 4097)]
    assert len({c.name for c in out}) == len(out)
    return out


_KEPT = {}


def reference(case, nthreads=16):
    """direct() of a case onto zeros: dict of hist, det, seen and tallies.  Kept and served again: the tests share it and leave it
    unchanged."""
    if case.name in _KEPT:
        return _KEPT[case.name]
    from tests.receive_cases import Case, oracle_of
    _, o = oracle_of(Case(case.name, case.scene, case.partition, np.zeros((0, 6)), 1, np.zeros((1, 3)), np.ones(1), 1, 1.0, 0))
    hist = np.zeros(case.shape, np.uint64)
    det = np.zeros((case.K, 2), np.uint64)
    centers, radii = case.receivers()
    seen, tallies = {}, {}
    direct(o, *case.source(), centers, radii, case.n_weight, case.n_bins, case.bin_len, case.frac_bits, hist, det, seen, tallies, nthreads)
    out = _KEPT[case.name] = dict(hist=hist, det=det, seen=seen, tallies=tallies)
    return out
