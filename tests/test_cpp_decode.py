"""The C++ mirror's decoding call (bindings/cpp/hare.hpp: Decode) through bindings/cpp/decode_example.cpp, in the manner of
tests/test_cpp_convolve.py: it compiles without a warning and its size checks refuse; on a GPU its output is the Python call's and the numpy
restatement's (tests/decode_ref.py) on the same inputs, value for value, and two output windows give what the one call gives."""
import os
import subprocess

import numpy as np
import pytest

import hare_amd as H
from tests.decode_ref import decode_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, C, N, O, T = 2, 4, 50, 2, 12


def build(tmp_path):
    exe = str(tmp_path / "hare_decode")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "bindings", "cpp"), os.path.join(ROOT, "bindings", "cpp", "decode_example.cpp"),
                           "-L", os.path.join(ROOT, "hare_amd"), "-lhare_hip", "-Wl,-rpath," + os.path.join(ROOT, "hare_amd"),
                           "-o", exe])
    return exe


def example_inputs():
    t, r = np.arange(N), np.arange(K * C)
    x = np.where(t & 1, -1.0, 1.0)[None, :] / (1 + r[:, None] + t[None, :])
    h = 0.125 * (np.arange(O * C * T) % 7) - 0.3
    return x.reshape(K, C, N), h.reshape(O, C, T)


def test_cpp_decode_size_checks(tmp_path, gpu_available):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    x, h = example_inputs()
    head = r.stdout.splitlines()[0].replace(",", "").split()
    assert head[:2] == ["in", f"{K * C * N}:"] and head[4:6] == ["h", f"{O * C * T}:"], r.stdout + r.stderr
    assert [float(v) for v in head[2:4] + head[6:8]] == [x[0, 0, 0], x[-1, -1, -1], h[0, 0, 0], h[-1, -1, -1]]
    assert "refused 4" in r.stdout
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device visible" in r.stdout and "decode:" not in r.stdout


@pytest.mark.gpu
def test_cpp_decode_on_gpu_matches_the_python_call_and_the_reference(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"decode: out {K * O * (N + T - 1)}, windows same 1" in r.stdout, r.stdout
    x, h = example_inputs()
    m = H.scenes.shoebox()
    g = H.Voxel_Grid([H.Topology(m.verts, m.nverts)], 8)
    out = g.decode(x, h)
    assert out.shape == (K, O, N + T - 1) and out.tobytes() == decode_ref(x, h).tobytes()
    line = [l for l in r.stdout.splitlines() if l.startswith("out:")][0]
    assert [float(v) for v in line.split()[1:]] == out.reshape(-1).tolist()
