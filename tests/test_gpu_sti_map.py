"""The STI-map recipe of INTEGRATION.md ("Receiver maps: a speech transmission index per receiver") end to end on the MI355X: a receiver
map over an audience plane, the source's rays emitted and traced with hare_receive_device, hare_hist_project_device behind it on the same
stream onto hare_amd.sti.mtf_vectors, and one STI value per receiver from the projections alone -- 29 sums per receiver and band come
down, never the histogram.  The histogram is downloaded here only to hold the projections against tests/project_ref.py."""
import numpy as np
import pytest

import hare_amd as H
from hare_amd import sti
from tests.project_ref import project_ref

pytestmark = pytest.mark.gpu

N_RAYS, CASTS, N_BINS, BIN_LEN, C_SOUND, FRAC, BANDS = 20_000, 30, 200, 1.715, 343.0, 30, 7          # 5 ms bins, one second


def test_a_map_yields_one_sti_value_per_receiver_without_the_histogram_leaving_the_device():
    import torch
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    g.set_absorption(np.tile(np.linspace(0.1, 0.4, BANDS), (m.verts.shape[0], 1)))          # more absorption towards 8 kHz
    g.set_source([2.0, 3.5, 1.7])
    centers, radii = H.Voxel_Grid.receiver_plane([0.5, 0.5], [9.5, 6.5], 1.2, 1.0, 0.4)
    K = centers.shape[0]
    g.set_receiver_map(centers, radii)
    table = sti.mtf_vectors(N_BINS, BIN_LEN, C_SOUND)                                       # int32 [29, n_bins]
    J = table.shape[0]

    n = N_RAYS
    d_rays = torch.empty(n * 6, dtype=torch.float64, device="cuda")
    d_state = torch.empty(n * (1 + BANDS), dtype=torch.float64, device="cuda")
    d_work = torch.zeros(H.Voxel_Grid.receive_work_bytes(n), dtype=torch.uint8, device="cuda")
    d_last = torch.zeros(n * 56, dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros(K * N_BINS * BANDS, dtype=torch.int64, device="cuda")
    d_det = torch.zeros(2 * K, dtype=torch.int64, device="cuda")
    d_coef = torch.from_numpy(table).to("cuda")
    d_proj = torch.empty(K * BANDS * J * 2, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    g.emit_device(n, d_rays.data_ptr(), d_state.data_ptr(), stream=stream)
    g.receive_device(n, d_rays.data_ptr(), CASTS, N_BINS, BIN_LEN, FRAC, d_state.data_ptr(), d_work.data_ptr(), d_last.data_ptr(),
                     d_hist.data_ptr(), d_det.data_ptr(), stream=stream)
    g.hist_project_device(K, N_BINS, BANDS, 1, d_hist.data_ptr(), J, d_coef.data_ptr(), d_proj.data_ptr(), stream=stream)
    proj = d_proj.cpu().numpy().view(np.uint64).reshape(K, BANDS, J, 2)                    # K x 7 x 29 x 16 bytes: all that comes down
    value = sti.sti(sti.mtf(proj))

    assert value.shape == (K,) and K == 70
    assert np.isfinite(value).all() and (value > 0.3).all() and (value < 1.0).all(), value
    assert value.max() - value.min() > 0.01                                                # a map, not a constant: the source is off-centre
    hist = d_hist.cpu().numpy().view(np.uint64).reshape(K, N_BINS, BANDS)                  # for the check alone
    assert hist.any(axis=(1, 2)).all()                                                     # every receiver was reached
    assert proj.tobytes() == project_ref(hist, table).tobytes()
