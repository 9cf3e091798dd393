"""The C++ mirror's first-order image sources (bindings/cpp/hare.hpp: ReceiveSource's `image`, ImageDevice, ImageWorkBytes) through
bindings/cpp/image_example.cpp, in the manner of tests/test_cpp_direct.py: it compiles without a warning, its size helper and its
argument checks answer as the header says; on a GPU its deposit is the Python call's on the same scene: the direct sound and one
reflection per wall of the cube, whatever the seed."""
import os
import subprocess

import numpy as np
import pytest

import hare_amd as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "hare_image")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "bindings", "cpp"), os.path.join(ROOT, "bindings", "cpp", "image_example.cpp"),
                           "-L", os.path.join(ROOT, "hare_amd"), "-lhare_hip", "-Wl,-rpath," + os.path.join(ROOT, "hare_amd"),
                           "-o", exe])
    return exe


def test_cpp_image_flag_size_and_refusals(tmp_path, gpu_available):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert "flag 2048, work bytes %d, max pairs %d" % (H.Voxel_Grid.image_work_bytes(1, 12, 64), 1 << 20) in r.stdout, r.stdout + r.stderr
    assert "refused 4" in r.stdout
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device visible" in r.stdout and "image:" not in r.stdout


@pytest.mark.gpu
def test_cpp_image_on_gpu_matches_the_python_call(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "image: detections 7, seeds agree" in r.stdout, r.stdout              # the direct sound and six walls
    c = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0], [0, 0, 2], [2, 0, 2], [2, 2, 2], [0, 2, 2]], np.float64)
    f = [[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6], [0, 5, 1], [0, 4, 5], [3, 2, 6], [3, 6, 7], [0, 3, 7], [0, 7, 4], [1, 5, 6], [1, 6, 2]]
    verts = np.zeros((12, 4, 3))
    verts[:, :3] = c[np.array(f)]
    g = H.Voxel_Grid([H.Topology(verts, np.full(12, 3, np.int32))], 4)
    g.set_receivers([[1.5, 0.75, 1.25]], [0.25]).set_absorption(np.full((12, 2), 0.2))
    g.set_source([1.0, 1.0, 1.0], power=[1.0, 0.5])
    hist, _, det, *_ = g.Receive_source(4096, 1, 16, 0.25, frac_bits=30, direct=True, image=True)
    words = [int(x) for x in [l for l in r.stdout.splitlines() if l.startswith("words:")][0].split()[1:]]
    assert words == hist.reshape(-1).tolist() and det.tolist() == [[7, 0]]
    only_direct = g.Receive_source(4096, 1, 16, 0.25, frac_bits=30, direct=True)[0]
    assert hist.sum() > only_direct.sum() and np.count_nonzero(hist[0, :, 0]) > 1
