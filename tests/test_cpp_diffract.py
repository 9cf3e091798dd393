"""The C++ mirror's first-order edge diffraction (bindings/cpp/hare.hpp: SetEdges, DiffractPaths, DiffractDevice, DiffractWorkBytes) through
bindings/cpp/diffract_example.cpp, in the manner of tests/test_cpp_image.py: it compiles without a warning, its size helper and its
argument checks answer as the header says; on a GPU its histogram is the Python call's on the same scene: one path over each free edge of
the screen for a receiver the direct sound does not reach."""
import os
import subprocess

import numpy as np
import pytest

import hare_amd as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "hare_diffract")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "bindings", "cpp"), os.path.join(ROOT, "bindings", "cpp", "diffract_example.cpp"),
                           "-L", os.path.join(ROOT, "hare_amd"), "-lhare_hip", "-Wl,-rpath," + os.path.join(ROOT, "hare_amd"),
                           "-o", exe])
    return exe


def test_cpp_diffract_size_edges_and_refusals(tmp_path, gpu_available):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert "work bytes %d, edges 3" % H.Voxel_Grid.diffract_work_bytes(1, 64) in r.stdout, r.stdout + r.stderr
    assert "refused 5, edges 3" in r.stdout                                       # a refused setter changes nothing
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device visible" in r.stdout and "diffract:" not in r.stdout


@pytest.mark.gpu
def test_cpp_diffract_on_gpu_matches_the_python_call(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "diffract: found 3, detections 3, direct detections 0" in r.stdout, r.stdout
    c = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0], [0, 0, 2], [2, 0, 2], [2, 2, 2], [0, 2, 2]], np.float64)
    f = [[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6], [0, 5, 1], [0, 4, 5], [3, 2, 6], [3, 6, 7], [0, 3, 7], [0, 7, 4], [1, 5, 6], [1, 6, 2]]
    verts = np.zeros((13, 4, 3))
    verts[:12, :3] = c[np.array(f)]
    verts[12] = [[1, 0.5, 0], [1, 1.5, 0], [1, 1.5, 1.25], [1, 0.5, 1.25]]
    g = H.Voxel_Grid([H.Topology(verts, np.array([3] * 12 + [4], np.int32))], 4)
    g.set_receivers([[1.625, 1.0, 0.375]], [0.125]).set_absorption(np.full((13, 2), 0.2))
    g.set_source([0.5, 1.0, 0.5], power=[1.0, 0.5])
    ends = [[[1, 0.5, 1.25], [1, 1.5, 1.25]], [[1, 0.5, 0], [1, 0.5, 1.25]], [[1, 1.5, 0], [1, 1.5, 1.25]]]
    g.set_edges(ends, [[12, -1]] * 3, [250.0 / 343.0, 1000.0 / 343.0])
    hist, det, found = g.Diffract_paths(4096, 16, 0.25, 64, frac_bits=30)
    words = [int(x) for x in [l for l in r.stdout.splitlines() if l.startswith("words:")][0].split()[1:]]
    assert found == 3 and words == hist.reshape(-1).tolist() and det.tolist() == [[3, 0]] and hist.any()
    assert (hist[0, :, 1] < hist[0, :, 0])[hist[0, :, 0] > 0].all()              # the higher band is attenuated more, at half the power
