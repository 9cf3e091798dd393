"""The C++ mirror's second-order image sources (bindings/cpp/hare.hpp: ReceiveSource's `image2`, Image2Device, Image2WorkBytes) through
bindings/cpp/image2_example.cpp, in the manner of tests/test_cpp_image.py: it compiles without a warning, its size helper and its argument
checks answer as the header says; on a GPU its three deposits are the Python call's on the same scene, whatever the seed."""
import os
import subprocess

import numpy as np
import pytest

import hare_amd as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "hare_image2")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "bindings", "cpp"), os.path.join(ROOT, "bindings", "cpp", "image2_example.cpp"),
                           "-L", os.path.join(ROOT, "hare_amd"), "-lhare_hip", "-Wl,-rpath," + os.path.join(ROOT, "hare_amd"),
                           "-o", exe])
    return exe


def test_cpp_image2_flag_size_and_refusals(tmp_path, gpu_available):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    want = "flag 65536, work bytes %d, max cands %d, max paths %d, prune 1" % (H.Voxel_Grid.image2_work_bytes(12, 132, 64), 1 << 22, 1 << 20)
    assert want in r.stdout, r.stdout + r.stderr
    assert "refused 5" in r.stdout
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device visible" in r.stdout and "image2:" not in r.stdout


@pytest.mark.gpu
def test_cpp_image2_on_gpu_matches_the_python_call(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "seeds agree" in r.stdout, r.stdout
    c = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0], [0, 0, 2], [2, 0, 2], [2, 2, 2], [0, 2, 2]], np.float64)
    f = [[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6], [0, 5, 1], [0, 4, 5], [3, 2, 6], [3, 6, 7], [0, 3, 7], [0, 7, 4], [1, 5, 6], [1, 6, 2]]
    verts = np.zeros((12, 4, 3))
    verts[:, :3] = c[np.array(f)]
    g = H.Voxel_Grid([H.Topology(verts, np.full(12, 3, np.int32))], 4)
    g.set_receivers([[1.5, 0.75, 1.25]], [0.25]).set_absorption(np.full((12, 2), 0.2))
    g.set_source([1.0, 1.0, 1.0], power=[1.0, 0.5])
    hist, _, det, *_ = g.Receive_source(4096, 1, 16, 0.25, frac_bits=30, direct=True, image=True, image2=True)
    words = [int(x) for x in [l for l in r.stdout.splitlines() if l.startswith("words:")][0].split()[1:]]
    assert words == hist.reshape(-1).tolist() and "image2: detections %d," % int(det.sum()) in r.stdout
    first = g.Receive_source(4096, 1, 16, 0.25, frac_bits=30, direct=True, image=True)
    assert det.sum() > first[2].sum() and hist.sum() > first[0].sum()       # the second order adds paths and energy
