"""The C++ mirror's direct sound (bindings/cpp/hare.hpp: ReceiveSource's `direct`, DirectDevice, DirectWorkBytes) through
bindings/cpp/direct_example.cpp, in the manner of tests/test_cpp_reduce.py: it compiles without a warning, its size helper and its
argument checks answer as the header says; on a GPU its deposit is the Python call's on the same scene, and f * n of the source's power."""
import os
import subprocess

import numpy as np
import pytest

import hare_amd as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "hare_direct")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "bindings", "cpp"), os.path.join(ROOT, "bindings", "cpp", "direct_example.cpp"),
                           "-L", os.path.join(ROOT, "hare_amd"), "-lhare_hip", "-Wl,-rpath," + os.path.join(ROOT, "hare_amd"),
                           "-o", exe])
    return exe


def test_cpp_direct_flag_size_and_refusals(tmp_path, gpu_available):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert "flag 1024, work bytes %d" % H.Voxel_Grid.direct_work_bytes(2) in r.stdout, r.stdout + r.stderr
    assert "refused 3" in r.stdout
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device visible" in r.stdout and "direct:" not in r.stdout


@pytest.mark.gpu
def test_cpp_direct_on_gpu_matches_the_python_call(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    # one deposit per receiver the source sees, whatever the seed; the source radiates into +x only, so the one behind it gets zero energy
    assert "direct: detections front 1, behind 1, seeds agree" in r.stdout, r.stdout
    c = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0], [0, 0, 2], [2, 0, 2], [2, 2, 2], [0, 2, 2]], np.float64)
    f = [[0, 1, 2], [0, 2, 3], [4, 6, 5], [4, 7, 6], [0, 5, 1], [0, 4, 5], [3, 2, 6], [3, 6, 7], [0, 3, 7], [0, 7, 4], [1, 5, 6], [1, 6, 2]]
    verts = np.zeros((12, 4, 3))
    verts[:, :3] = c[np.array(f)]
    g = H.Voxel_Grid([H.Topology(verts, np.full(12, 3, np.int32))], 4)
    g.set_receivers([[1.5, 1.0, 1.0], [0.5, 1.0, 1.0]], [0.25, 0.25]).set_absorption(np.full((12, 2), 0.2))
    gain = np.zeros((6, 1, 1, 2))
    gain[0] = 1.0
    g.set_source([1.0, 1.0, 1.0], power=[1.0, 0.5], gain=gain)
    hist, _, det, *_ = g.Receive_source(4096, 1, 16, 0.25, frac_bits=30, direct=True)
    words = [int(x) for x in [l for l in r.stdout.splitlines() if l.startswith("words:")][0].split()[1:]]
    assert words == hist[0, 2].tolist() and hist.sum() == sum(words)
    assert det.tolist() == [[1, 0], [1, 0]] and not hist[1].any()
    fshare = (0.5 * 0.25) / (1.0 + np.sqrt(0.75))
    assert words[0] == int(np.rint(fshare * 4096 * 2.0 ** 30)) and words[1] == int(np.rint(0.5 * fshare * 4096 * 2.0 ** 30))
