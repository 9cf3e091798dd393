"""The C++ mirror's receiver calls (bindings/cpp/hare.hpp) on a scene of two topologies whose second has an absorption table of 8 bands:
the wrapper sizes the histogram and the state from the scene's own record of that topology's bands ("bands:<top>"), so the library's
K x n_bins x 8 words land inside the vector; short centre and alpha vectors are refused before the library reads them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path):
    exe = str(tmp_path / "hare_receivers")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "bindings", "cpp"), os.path.join(ROOT, "bindings", "cpp", "receivers_example.cpp"),
                           "-L", os.path.join(ROOT, "hare_amd"), "-lhare_hip", "-Wl,-rpath," + os.path.join(ROOT, "hare_amd"),
                           "-o", exe])
    return exe


def test_cpp_receivers_size_from_the_topologys_bands(tmp_path, gpu_available):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert "receivers 2, bands 1 / 8" in r.stdout, r.stdout + r.stderr
    assert "refused 3" in r.stdout
    if not gpu_available:
        assert r.returncode == 2 and "no HIP device visible" in r.stdout and "receive:" not in r.stdout


@pytest.mark.gpu
def test_cpp_receivers_on_gpu(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    # 2 receivers x 16 bins x 8 bands; state (1 + 8) x 6.  Each ray passes receiver 0 in each of its 3 casts (in cast 0 at its own origin:
    # s = 0, bin 0, E = 1 -> 2^20 per band and ray); receiver 1 lies off every ray.
    assert "receive: hist 256, state 54, detections 18 0, band 7 of receiver 0 bin 0: 6291456" in r.stdout, r.stdout
