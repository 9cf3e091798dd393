"""hare_receive_source_reduced / hare_receive_batch_reduced on the MI355X (include/hare_hip.h, "receivers", "Reduction"): the loop of the
parent call with the histogram kept on the device and reduced there.  In the shoebox under Voxel_Grid(8), with a 12 x 12 receiver map,
three bands, an absorption and a scattering table, 4 096 rays and 6 casts: sums and crossings equal, byte for byte, the restatement
(tests/reduce_ref.py) of the histogram the plain call returns; detections, state and counters equal the plain call's -- from the
source and from caller rays, with four channels, with air-absorption weights, and with three receivers through set_receivers."""
import numpy as np
import pytest

import hare_amd as H
from tests.receive_harness import same_bits
from tests.reduce_ref import reduce_ref
from tests.test_gpu_receivers import alpha_table
from tests.test_gpu_scattering import sigma_table

pytestmark = pytest.mark.gpu

N, CASTS, B = 4096, 6, 3
N_BINS, BIN_LEN, FRAC = 64, 0.75, 40
WINDOWS = [(0, N_BINS), (0, 7), (7, N_BINS), (3, 40)]
LEVELS = H.decay_levels(-np.arange(5.0, 36.0))
AIR = H.air_weights([0.001, 0.01, 0.05], BIN_LEN, N_BINS)


@pytest.fixture(scope="module")
def parts():
    """The map scene and the linear 3-receiver scene, tables, source and seed set."""
    m = H.scenes.shoebox()
    T = H.Topology(m.verts, m.nverts)
    centers, radii = H.Spatial_Partition.receiver_plane((2.0, 0.5), (7.75, 6.25), 1.2, 0.5, 0.3)
    assert centers.shape == (144, 3)
    out = {}
    for name in ("map", "linear"):
        g = H.Voxel_Grid([T], 8)
        if name == "map":
            g.set_receiver_map(centers, radii)
        else:
            g.set_receivers(centers[[0, 70, 143]], [0.8, 0.9, 1.0])
        g.set_absorption(alpha_table(T.Polygon_Count, B)).set_scattering(sigma_table(T.Polygon_Count, B))
        g.set_source(np.array([0.31, 0.42, 0.37]) * np.asarray(m.size), power=[1.0, 0.5, 2.0]).set_option("scatter_seed", 11)
        out[name] = g
    return out, H.scenes.burst_rays(N, m.size)


MODES = {"source": dict(), "batch": dict(batch=True), "directional": dict(directional=True), "batch-directional": dict(batch=True, directional=True),
         "weights": dict(weight=AIR), "linear": dict(scene="linear"), "linear-batch-weights": dict(scene="linear", batch=True, weight=AIR),
         "levels-only": dict(windows=None), "windows-only": dict(levels=None, directional=True)}


@pytest.mark.parametrize("mode", MODES, ids=list(MODES))
def test_reduced_call_equals_the_reduction_of_the_plain_calls_histogram(parts, mode):
    scenes, rays = parts
    kw = dict(scene="map", batch=False, directional=False, weight=None, windows=WINDOWS, levels=LEVELS)
    kw.update(MODES[mode])
    g = scenes[kw["scene"]]
    reduce = dict(windows=kw["windows"], levels=kw["levels"], weight=kw["weight"])
    more = dict(frac_bits=FRAC, directional=kw["directional"])
    if kw["batch"]:
        plain = g.Receive_batch(rays, CASTS, N_BINS, BIN_LEN, frac_bits=FRAC, directional=kw["directional"])
        got = g.Receive_batch_reduced(rays, CASTS, N_BINS, BIN_LEN, **reduce, **more)
    else:
        plain = g.Receive_source(N, CASTS, N_BINS, BIN_LEN, frac_bits=FRAC, directional=kw["directional"])
        got = g.Receive_source_reduced(N, CASTS, N_BINS, BIN_LEN, **reduce, **more)
    hist, _, det, state, ctr = plain
    assert hist.shape[:3] == (144 if kw["scene"] == "map" else 3, N_BINS, B) and np.count_nonzero(hist) > 100      # not vacuous
    want_sums, want_cross = reduce_ref(hist, kw["windows"] or [], [] if kw["levels"] is None else kw["levels"], kw["weight"])
    sums, cross, det2, state2, ctr2 = got
    assert same_bits(sums, want_sums) is None, same_bits(sums, want_sums)
    assert same_bits(cross, want_cross) is None, same_bits(cross, want_cross)
    assert same_bits(det2, det) is None and same_bits(state2, state) is None and ctr2 == ctr
    if kw["levels"] is not None:
        assert len(np.unique(want_cross)) > 3                                                                        # the decay is resolved
