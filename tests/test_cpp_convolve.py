"""The C++ mirror's convolution call (bindings/cpp/hare.hpp: Convolve) through bindings/cpp/convolve_example.cpp, in the manner of
tests/test_cpp_render.py: it compiles without a warning and its size checks refuse; on a GPU its output is the Python call's and the numpy
restatement's (tests/convolve_ref.py) on the same inputs, value for value, and two output windows give what the one call gives."""
import os
import subprocess

import numpy as np
import pytest

import hare_amd as H
from tests.convolve_ref import convolve_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, N, L = 3, 50, 20


def build(tmp_path):
    exe = str(tmp_path / "hare_convolve")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "bindings", "cpp"), os.path.join(ROOT, "bindings", "cpp", "convolve_example.cpp"),
                           "-L", os.path.join(ROOT, "hare_amd"), "-lhare_hip", "-Wl,-rpath," + os.path.join(ROOT, "hare_amd"),
                           "-o", exe])
    return exe


def example_inputs():
    t = np.arange(N)
    ir = np.where(t & 1, -1.0, 1.0)[None, :] / (1 + np.arange(R)[:, None] + t[None, :])
    return ir, 0.25 * np.arange(L) - 1.0


def test_cpp_convolve_size_checks(tmp_path, gpu_available):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    ir, x = example_inputs()
    head = r.stdout.splitlines()[0].replace(",", "").split()
    assert head[:2] == ["ir", f"{R * N}:"] and head[4:6] == ["x", f"{L}:"], r.stdout + r.stderr
    assert [float(v) for v in head[2:4] + head[6:8]] == [ir[0, 0], ir[-1, -1], x[0], x[-1]]
    assert "refused 3" in r.stdout
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device visible" in r.stdout and "convolve:" not in r.stdout


@pytest.mark.gpu
def test_cpp_convolve_on_gpu_matches_the_python_call_and_the_reference(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"convolve: out {R * (N + L - 1)}, windows same 1" in r.stdout, r.stdout
    ir, x = example_inputs()
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    out = g.convolve(ir, x)
    assert out.shape == (R, N + L - 1) and out.tobytes() == convolve_ref(ir, x).tobytes()
    line = [l for l in r.stdout.splitlines() if l.startswith("out:")][0]
    assert [float(v) for v in line.split()[1:]] == out.reshape(-1).tolist()
